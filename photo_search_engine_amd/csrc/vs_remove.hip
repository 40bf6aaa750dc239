// vs_remove.hip -- exact row removal on the flat index (include/vs.h "row removal").
//
// faiss IndexFlat::remove_ids compacts its row-major array with a host memmove.  Here the rows live
// in HBM as 256-row chunk-major tiles with their norms (sqn), the int8 screen copy and its group
// means beside them, so the compaction runs on the device:
//   * the removal bitmap is complemented (k_remove_complement) and compacted by the selectors'
//     k_sel_count / k_sel_compact into the ascending list of kept ids: new row j = old row src[j],
//     src[j] >= j;
//   * rows before the tile of the first removed id are not touched; from there on the destination
//     tiles are rebuilt in ascending batches through a bounce buffer: k_remove_gather writes a
//     batch's new tiles into the buffer (as final tiles), k_remove_place copies the buffer over the
//     batch's tiles.  Both run on one stream.  A later batch reads only rows src[j] >= j >= the end
//     of this batch's destination range, which no earlier batch has written, and no kernel reads
//     and writes the live array: no ordering between workgroups is needed;
//   * a row's piece of a chunk is one 128 B line: 8 lanes move 16 B each, a wave moves 8 rows of one
//     chunk per instruction (whole lines on both sides), one workgroup builds one destination tile;
//     sqn rides along (4 B per row); the last tile's rows past the new count are zeroed, as a fresh
//     allocation has them;
//   * the int8 copy is requantised from the first removed row on (from its group's first row where
//     group means exist: the groups re-form), by the calls every add makes; max ||x||^2 is
//     recomputed over the survivors (k_remove_maxsq), the int8 maxima stay upper bounds (the
//     untouched head's values plus the requantised rows').
#include "vs_index.h"

using namespace vs;

namespace vs {

constexpr int RM_THREADS = 512;           // k_remove_gather: 8 waves per destination tile
constexpr int RM_NW = RM_THREADS / 64;
constexpr int RM_ROWS = 8;                // rows a wave moves per instruction (8 lanes x 16 B each)
constexpr int RM_U = 4;                   // lines in flight per lane
constexpr int RM_PIECE = CHB / RM_ROWS;   // 16 B
static_assert(RM_PIECE == 16 && TR % (RM_ROWS * RM_NW) == 0, "k_remove_gather: 16 B pieces, whole row groups");

__global__ void __launch_bounds__(256) k_remove_complement(u64* __restrict__ bits, int64_t nwords) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nwords) bits[i] = ~bits[i];
}

__global__ void __launch_bounds__(RM_THREADS) k_remove_gather(const uint8_t* __restrict__ data, int64_t tb, int nchunks,
                                                              const uint32_t* __restrict__ src, int64_t n_new,
                                                              int64_t t0, uint8_t* __restrict__ stage,
                                                              const float* __restrict__ sqn,
                                                              float* __restrict__ sqn_out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int sub = lane / RM_ROWS, piece = lane % RM_ROWS;
    const int64_t row0 = (t0 + blockIdx.x) * TR;  // first new row of this destination tile
    uint8_t* dst_tile = stage + (int64_t)blockIdx.x * tb;
    constexpr int64_t CS = (int64_t)TR * CHB;  // bytes of one chunk of a tile
    for (int rg = wid; rg < TR / RM_ROWS; rg += RM_NW) {
        const int r = rg * RM_ROWS + sub;
        const bool live = row0 + r < n_new;
        const uint32_t s = live ? src[row0 + r] : 0u;
        const uint8_t* sp = data + (int64_t)(s / TR) * tb + (int64_t)(s % TR) * CHB + piece * RM_PIECE;
        uint8_t* dp = dst_tile + r * CHB + piece * RM_PIECE;
        for (int c = 0; c < nchunks; c += RM_U) {
            uint4 v[RM_U];
#pragma unroll
            for (int u = 0; u < RM_U; ++u) {
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                if (live && c + u < nchunks) v[u] = *(const uint4*)(sp + (c + u) * CS);
            }
#pragma unroll
            for (int u = 0; u < RM_U; ++u)
                if (c + u < nchunks) *(uint4*)(dp + (c + u) * CS) = v[u];
        }
    }
    if (threadIdx.x < TR) {
        const int64_t j = row0 + threadIdx.x;
        sqn_out[(int64_t)blockIdx.x * TR + threadIdx.x] = j < n_new ? sqn[src[j]] : 0.0f;
    }
}

// n16 16-byte pieces of the staged tiles, then s16 of the staged sqn entries, each to its place
__global__ void __launch_bounds__(256) k_remove_place(const uint4* __restrict__ stage, int64_t n16,
                                                      uint4* __restrict__ data, const uint4* __restrict__ sqn_stage,
                                                      int64_t s16, uint4* __restrict__ sqn) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16 + s16; i += stride) {
        if (i < n16) data[i] = stage[i];
        else sqn[i - n16] = sqn_stage[i - n16];
    }
}

__global__ void __launch_bounds__(256) k_remove_maxsq(const float* __restrict__ sqn, int64_t n,
                                                      unsigned* __restrict__ maxsq) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    float m = 0.0f;  // (sqn >= 0: the fp32 bits order as the values do)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) m = fmaxf(m, sqn[i]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxsq, __float_as_uint(m));
}

hipError_t launch_remove_complement(uint64_t* bits, int64_t nwords, hipStream_t st) {
    if (!bits || nwords <= 0 || (nwords + 255) / 256 > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_remove_complement, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, (u64*)bits, nwords);
    return hipGetLastError();
}

hipError_t launch_remove_gather(const uint8_t* data, int64_t tile_bytes, int nchunks, const uint32_t* src,
                                int64_t n_new, int64_t t0, int64_t nt, uint8_t* stage, const float* sqn,
                                float* sqn_out, hipStream_t st) {
    if (!data || !src || !stage || !sqn || !sqn_out || nchunks <= 0 || tile_bytes != (int64_t)nchunks * TR * CHB ||
        n_new <= 0 || t0 < 0 || nt <= 0 || nt > 0x7FFFFFFF || (t0 + nt - 1) * TR >= n_new)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_remove_gather, dim3((unsigned)nt), dim3(RM_THREADS), 0, st, data, tile_bytes, nchunks, src, n_new,
                       t0, stage, sqn, sqn_out);
    return hipGetLastError();
}

hipError_t launch_remove_place(const uint8_t* stage, int64_t tile_bytes, int64_t t0, int64_t nt, uint8_t* data,
                               const float* sqn_stage, float* sqn, hipStream_t st) {
    if (!stage || !data || !sqn_stage || !sqn || tile_bytes <= 0 || tile_bytes % 16 != 0 || t0 < 0 || nt <= 0)
        return hipErrorInvalidValue;
    const int64_t n16 = nt * tile_bytes / 16, s16 = nt * TR * (int64_t)sizeof(float) / 16;
    const int64_t blocks = std::min<int64_t>((n16 + s16 + 1023) / 1024, 8192);
    hipLaunchKernelGGL(k_remove_place, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)stage, n16,
                       (uint4*)(data + t0 * tile_bytes), (const uint4*)sqn_stage, s16, (uint4*)(sqn + t0 * TR));
    return hipGetLastError();
}

hipError_t launch_remove_maxsq(const float* sqn, int64_t n, unsigned* maxsq, hipStream_t st) {
    if (!sqn || n <= 0 || !maxsq) return hipErrorInvalidValue;
    const int64_t blocks = std::min<int64_t>((n + 1023) / 1024, 1024);
    hipLaunchKernelGGL(k_remove_maxsq, dim3((unsigned)blocks), dim3(256), 0, st, sqn, n, maxsq);
    return hipGetLastError();
}

}  // namespace vs

namespace {

constexpr int64_t kDefaultRemoveStaging = 256ll << 20;
std::atomic<int64_t> g_remove_staging{kDefaultRemoveStaging};

}  // namespace

extern "C" {

int vs_set_remove_staging_bytes(int64_t bytes) {
    return guarded([&] {
        if (bytes < 1) throw VsError(VS_ERR_ARG, "remove staging bytes must be >= 1 (the floor is one row tile)");
        g_remove_staging.store(bytes);
    });
}

int vs_remove_ids(vs_index* ix, const uint8_t* bitmap, int64_t nbytes, int64_t* n_removed) {
    return guarded([&] {
        check_index(ix);
        if (n_removed) *n_removed = 0;
        std::unique_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        const int64_t n = ix->ntotal;
        const int64_t need = (n + 7) / 8;
        if (nbytes < need || (need > 0 && !bitmap))
            throw VsError(VS_ERR_ARG, "removal bitmap too short: " + std::to_string(need) + " bytes cover ntotal");
        // rows to remove and the first of them, bits at or past ntotal masked off
        int64_t removed = 0, f = -1;
        for (int64_t i = 0; i < need; ++i) {
            unsigned b = bitmap[i];
            if (i == need - 1 && (n & 7)) b &= (1u << (n & 7)) - 1u;
            if (!b) continue;
            if (f < 0) f = i * 8 + __builtin_ctz(b);
            removed += __builtin_popcount(b);
        }
        if (removed == 0) return;  // nothing moves, nothing is invalidated
        const int64_t n_new = n - removed;
        hipStream_t st = ix->own;
        if (n_new == 0) {  // every row: the state vs_reset leaves (capacity kept)
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemsetAsync(ix->d_maxsq, 0, sizeof(unsigned), st));
            reset_i8_stats(ix, st);
            HIP_CHECK(hipStreamSynchronize(st));
            ix->ntotal = 0;
            ix->reset_gen.fetch_add(1);
            ix->maxsq = 0.0f;
            ix->i8_bmax = 0.0f;
            ix->i8_res = false;
            if (n_removed) *n_removed = removed;
            return;
        }
        // every allocation before anything moves: a failure here leaves the index as it was
        const int64_t tb = tile_bytes(ix->dpad, ix->dtype);
        const int nchunks = (int)(tb / ((int64_t)TR * CHB));
        const int64_t t_first = f / TR, t_end = (n_new + TR - 1) / TR;  // destination tiles to rebuild
        const int64_t tiles = std::max<int64_t>(t_end - t_first, 0);
        const int64_t B = std::min(std::max<int64_t>(g_remove_staging.load() / tb, 1), std::max<int64_t>(tiles, 1));
        const int64_t nwords = (n + 63) / 64;
        const size_t cnt_off = (size_t)round_up(sel_compact_groups(n) * (int64_t)sizeof(unsigned), 8);
        DevBuf bits, ids, tmp, stage;  // (counted in vs_device_bytes_live, freed as the call returns)
        bits.ensure((size_t)nwords * 8);
        ids.ensure((size_t)n_new * sizeof(uint32_t));
        tmp.ensure(cnt_off + 8);
        if (tiles > 0) stage.ensure((size_t)B * (size_t)(tb + TR * (int64_t)sizeof(float)));
        // device-API searches may still be queued on other streams (they return before their kernels
        // run; the exclusive lock only orders host calls): they finish before a row moves
        HIP_CHECK(hipDeviceSynchronize());
        try {
            // the kept ids, ascending: the complement of the bitmap, compacted as a selector is
            HIP_CHECK(hipMemsetAsync(bits.p, 0, (size_t)nwords * 8, st));
            HIP_CHECK(hipMemcpyAsync(bits.p, bitmap, (size_t)need, hipMemcpyHostToDevice, st));
            HIP_CHECK(launch_remove_complement(bits.as<uint64_t>(), nwords, st));
            unsigned long long* cnt_d = (unsigned long long*)((uint8_t*)tmp.p + cnt_off);
            HIP_CHECK(launch_sel_compact(bits.as<uint64_t>(), n, tmp.as<unsigned>(), ids.as<uint32_t>(), n_new, cnt_d, st));
            unsigned long long cnt_h = 0;
            HIP_CHECK(hipMemcpyAsync(&cnt_h, cnt_d, sizeof(cnt_h), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if ((int64_t)cnt_h != n_new) throw VsError(VS_ERR_INTERNAL, "removal: kept-row count mismatch");
            float* sqn_stage = tiles > 0 ? (float*)((uint8_t*)stage.p + (size_t)B * tb) : nullptr;
            for (int64_t t = t_first; t < t_end; t += B) {
                const int64_t nt = std::min(B, t_end - t);
                HIP_CHECK(launch_remove_gather(ix->data, tb, nchunks, ids.as<uint32_t>(), n_new, t, nt,
                                               stage.as<uint8_t>(), ix->sqn, sqn_stage, st));
                HIP_CHECK(launch_remove_place(stage.as<uint8_t>(), tb, t, nt, ix->data, sqn_stage, ix->sqn, st));
            }
            // the int8 copy: codes and bounds of every row that moved; with group means the groups
            // re-form from the first removed row's group on
            if (ix->screen == VS_SCREEN_I8) {
                const int64_t r0 = ix->gmean ? f / I8_GROUP_ROWS * I8_GROUP_ROWS : f;
                if (n_new > r0) quantize_rows(ix, r0, n_new - r0, st);
            }
            // max ||x||^2 over the survivors (the value a fresh index of them holds)
            HIP_CHECK(hipMemsetAsync(ix->d_maxsq, 0, sizeof(unsigned), st));
            HIP_CHECK(launch_remove_maxsq(ix->sqn, n_new, ix->d_maxsq, st));
            HIP_CHECK(hipStreamSynchronize(st));
        } catch (...) {
            (void)hipStreamSynchronize(st);  // the buffers are freed behind the queued work
            throw;
        }
        ix->ntotal = n_new;
        ix->reset_gen.fetch_add(1);  // (selectors and graphs made before this are stale)
        refresh_maxsq(ix);
        if (n_removed) *n_removed = removed;
    });
}

}  // extern "C"

// vs_selscan.hip -- exact filtered search: id selectors on the flat index (include/vs.h "selectors").
//
// faiss answers "the k nearest among these rows" with SearchParameters(sel=IDSelectorBitmap(...)),
// which IndexFlat honours; the reference product has no such call and over-fetches instead
// (core/searcher.py:771-820, :887, :573-603, :931-936 of the reference).  Three kernels:
//   * k_sel_count / k_sel_compact: the device bitmap (faiss's layout, bit i of byte i >> 3) -> the
//     ascending uint32 list of the allowed ids of [0, n_sel) and their count.  A workgroup owns
//     SC_WORDS 64-bit words; the counts of the workgroups before it are summed (the "scan" of the
//     per-workgroup sums), the waves' counts inside it go through LDS, and inside a wave each 64-bit
//     word is a ballot: lane l owns bit l and writes id 64 w + l at the word's offset plus
//     lane_prefix(word).  Bits at or past n_sel are masked off the last word.
//   * k_sel_scan: k_full_scan's streaming exact top-k (fs_scan_body, vs_scan.h) driven by the id
//     list: workgroup b takes list positions [m b / G, m (b + 1) / G) (grid y: the queries are
//     dealt over query slices when the list fills few workgroups), each wave gathers its RR
//     listed rows (one 128 B line per row and chunk, as the refine does).  The list ascends, so the
//     tie argument of the full scan holds unchanged: the k lowest allowed ids among equal scores.
//   * k_sel_take: the overfetch tier -- per query, the allowed entries of an exact unfiltered
//     top-k' (order kept), the first k of them, and how many were found.
#include "vs_scan.h"

namespace vs {

constexpr int SC_THREADS = 256;
constexpr int SC_NW = SC_THREADS / 64;
constexpr int SC_ROUNDS = 4;                                // 64-word rounds per wave
constexpr int SC_WAVE_WORDS = 64 * SC_ROUNDS;               // words of one wave
constexpr int SC_WORDS = SC_NW * SC_WAVE_WORDS;             // words of one workgroup (65,536 ids)

// word wi of the bitmap with the bits at or past n_sel cleared (the host count masks the same way)
__device__ __forceinline__ u64 sel_word(const u64* __restrict__ bits, int64_t wi, int64_t n_sel) {
    const int64_t nw = (n_sel + 63) >> 6;
    if (wi >= nw) return 0ull;
    u64 w = bits[wi];
    const int tail = (int)(n_sel & 63);
    if (wi == nw - 1 && tail) w &= (1ull << tail) - 1ull;
    return w;
}

__global__ void __launch_bounds__(SC_THREADS) k_sel_count(const u64* __restrict__ bits, int64_t n_sel,
                                                          unsigned* __restrict__ wgsum) {
    __shared__ int wtot[SC_NW];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t w0 = ((int64_t)blockIdx.x * SC_NW + wid) * SC_WAVE_WORDS;
    int c = 0;
#pragma unroll
    for (int r = 0; r < SC_ROUNDS; ++r) c += __popcll(sel_word(bits, w0 + r * 64 + lane, n_sel));
    c = wave_sum_i(c);
    if (lane == 0) wtot[wid] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < SC_NW; ++i) t += wtot[i];
        wgsum[blockIdx.x] = (unsigned)t;
    }
}

// ids [cap]: the host's count of the same bitmap (no store past it); count: the device's total
__global__ void __launch_bounds__(SC_THREADS) k_sel_compact(const u64* __restrict__ bits, int64_t n_sel,
                                                            const unsigned* __restrict__ wgsum,
                                                            uint32_t* __restrict__ ids, int64_t cap,
                                                            unsigned long long* __restrict__ count) {
    __shared__ unsigned long long bsum[SC_NW];
    __shared__ int wtot[SC_NW];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int b = blockIdx.x;
    // ids of the workgroups before this one
    unsigned long long part = 0;
    for (int g = threadIdx.x; g < b; g += SC_THREADS) part += wgsum[g];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) part += __shfl_xor(part, s, 64);
    const int64_t w0 = ((int64_t)b * SC_NW + wid) * SC_WAVE_WORDS;
    u64 word[SC_ROUNDS];
    int c = 0;
#pragma unroll
    for (int r = 0; r < SC_ROUNDS; ++r) {
        word[r] = sel_word(bits, w0 + r * 64 + lane, n_sel);
        c += __popcll(word[r]);
    }
    c = wave_sum_i(c);
    if (lane == 0) {
        bsum[wid] = part;
        wtot[wid] = c;
    }
    __syncthreads();
    unsigned long long base = 0;
    int wg_total = 0;
    for (int i = 0; i < SC_NW; ++i) {
        base += bsum[i];
        if (i < wid) base += (unsigned long long)wtot[i];
        wg_total += wtot[i];
    }
    if (b == (int)gridDim.x - 1 && threadIdx.x == 0) {
        unsigned long long prior = 0;
        for (int i = 0; i < SC_NW; ++i) prior += bsum[i];
        *count = prior + (unsigned long long)wg_total;
    }
#pragma unroll
    for (int r = 0; r < SC_ROUNDS; ++r) {
        const int pc = __popcll(word[r]);
        int incl = pc;  // inclusive scan of the round's 64 counts
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int o = __shfl_up(incl, s, 64);
            if (lane >= s) incl += o;
        }
        const int excl = incl - pc;
        const int round_total = __shfl(incl, 63, 64);
        if (round_total) {  // (wave-uniform)
            for (int j = 0; j < 64; ++j) {
                const u64 wj = __shfl(word[r], j, 64);
                const int oj = __shfl(excl, j, 64);
                if ((wj >> lane) & 1ull) {
                    const unsigned long long pos = base + (unsigned long long)(oj + lane_prefix(wj));
                    if ((int64_t)pos < cap) ids[pos] = (uint32_t)((w0 + r * 64 + j) * 64 + lane);
                }
            }
        }
        base += (unsigned long long)round_total;
    }
}

int64_t sel_compact_groups(int64_t n_sel) {
    const int64_t nw = (n_sel + 63) >> 6;
    return std::max<int64_t>(1, (nw + SC_WORDS - 1) / SC_WORDS);
}

hipError_t launch_sel_compact(const uint64_t* bits, int64_t n_sel, unsigned* wgsum, uint32_t* ids, int64_t cap,
                              unsigned long long* count, hipStream_t st) {
    if (!bits || n_sel <= 0 || !wgsum || !ids || cap < 0 || !count) return hipErrorInvalidValue;
    const int64_t G = sel_compact_groups(n_sel);
    if (G > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sel_count, dim3((unsigned)G), dim3(SC_THREADS), 0, st, (const u64*)bits, n_sel, wgsum);
    hipLaunchKernelGGL(k_sel_compact, dim3((unsigned)G), dim3(SC_THREADS), 0, st, (const u64*)bits, n_sel,
                       (const unsigned*)wgsum, ids, cap, count);
    return hipGetLastError();
}

// ---- the list-driven scan ------------------------------------------------------------------------
template <int DT, int METRIC, bool QLDS>
__global__ void __launch_bounds__(FS_THREADS) k_sel_scan(FullScanArgs a, int KL, const uint32_t* __restrict__ ids,
                                                         int64_t m) {
    fs_scan_body<DT, METRIC, QLDS, true>(a, KL, ids, m);
}

hipError_t launch_sel_scan(const FullScanArgs& a, const uint32_t* ids, int64_t m, int qy, hipStream_t st) {
    if (qy < 1 || qy > a.nq || qy > 65535 || m < 0 || (m > 0 && !ids)) return hipErrorInvalidValue;
    return fs_launch_scan(a, 1, true, qy, st,
                          [](auto dt, auto metric, auto qlds, auto) { return k_sel_scan<dt, metric, qlds>; }, ids, m);
}

// ---- the overfetch tier's filter ------------------------------------------------------------------
// One wave per query: 64 entries of the unfiltered list at a time, the allowed ones ballot and take
// consecutive output slots (order kept) until k are written.
__global__ void __launch_bounds__(64) k_sel_take(SelTakeArgs a) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const int64_t* Iq = a.I_in + (size_t)q * a.kp;
    int cnt = 0;
    for (int j0 = 0; j0 < a.kp && cnt < a.k; j0 += 64) {
        const int j = j0 + lane;
        const int64_t id = j < a.kp ? Iq[j] : -1;
        const bool ok = id >= 0 && id < a.n_sel && ((a.bits[id >> 6] >> (id & 63)) & 1ull);
        const u64 mask = __ballot(ok);
        const int pos = cnt + lane_prefix(mask);
        if (ok && pos < a.k) {
            const size_t o = (size_t)q * a.k + pos;
            a.I[o] = id;
            if (a.D) a.D[o] = a.D_in[(size_t)q * a.kp + j];
            if (a.S64) a.S64[o] = a.S_in[(size_t)q * a.kp + j];
        }
        cnt += __popcll(mask);
    }
    cnt = min(cnt, a.k);
    for (int j = cnt + lane; j < a.k; j += 64) {
        const size_t o = (size_t)q * a.k + j;
        a.I[o] = -1;
        if (a.D) a.D[o] = a.metric == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
        if (a.S64) a.S64[o] = a.metric == METRIC_L2 ? 1.7976931348623157e308 : -1.7976931348623157e308;
    }
    if (lane == 0) {
        a.found[q] = cnt;
        // proven: the unfiltered list is exact and totally ordered, so its allowed entries are the
        // best allowed rows -- k of them, or all of them when the list holds every row
        a.cert_out[q] = (a.cert_in[q] != 0 && (cnt >= a.k || a.exhaustive)) ? 1 : 0;
    }
}

hipError_t launch_sel_take(const SelTakeArgs& a, int nq, hipStream_t st) {
    if (nq <= 0 || a.k <= 0 || a.kp < a.k || !a.bits || !a.I_in || !a.I || !a.found || !a.cert_in || !a.cert_out ||
        (a.D && !a.D_in) || (a.S64 && !a.S_in))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sel_take, dim3(nq), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace vs

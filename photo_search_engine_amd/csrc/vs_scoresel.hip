// vs_scoresel.hip -- exact score selectors: an id selector built on the device from a range predicate
// (include/vs.h "score selectors").
//
// The scoring kernels are the range search's (vs_range_scan.h) with the bit sink: the scan's K loop, its
// exact_score_rows call and its predicate are the same code, and a row that passes sets one bit.
//   * k_range_scan / k_range_refine with RsBitSink, over launch_facet_scan's dtype x metric x QLDS x SEL grid.
//   * k_bits_fold (mode ALL): acc[w] &= the AND of the block's nqb per-query bitmaps; one thread per word,
//     the loop over the queries reads consecutive words across the wave.
//   * k_bits_finish: out = (negate ? ~acc : acc) & members, the last word masked to n_sel, and the popcount
//     of the result added to one 64-bit total (one device atomic per workgroup).
//   * k_bits_op: vs_sel_combine's AND / OR / ANDNOT / NOT over two selectors' bitmaps, each operand read
//     as zero at and past its own n_sel; the same masking and popcount.
// Every store is to a word below ceil(n_sel / 64) of a bitmap the host sized.
#include "vs_range_scan.h"

namespace vs {

static bool bits_args_ok(const RangeArgs& a, const BitsArgs& b) {
    return a.self_mode == VS_SELF_KEEP && a.row0 == 0 && b.bits &&
           (b.stride_words == 0 || b.stride_words >= (a.n_valid + 63) >> 6);
}

hipError_t launch_bits_scan(const RangeArgs& a, const BitsArgs& b, int G, int qy, const uint32_t* ids, int64_t m,
                            hipStream_t st) {
    if (!bits_args_ok(a, b)) return hipErrorInvalidValue;
    return rs_launch_scan<RsBitSink, false>(a, {b.bits, b.stride_words}, 0, 0, G, qy, ids, m, st);
}

hipError_t launch_bits_refine(const RangeArgs& a, const BitsArgs& b, const u64* glist, const int* gcnt, int lcap, int ny,
                              hipStream_t st) {
    if (!bits_args_ok(a, b)) return hipErrorInvalidValue;
    return rs_launch_refine<RsBitSink, false>(a, {b.bits, b.stride_words}, glist, gcnt, lcap, ny, st);
}

// ---- bitmap kernels ---------------------------------------------------------------------------------
constexpr int BW_THREADS = 256;
constexpr int BW_NW = BW_THREADS / 64;

// word wi of a bitmap over rows [0, n): zero at and past word ceil(n / 64), the last word's bits at and
// past n cleared (k_sel_compact's masking); null with n > 0 = every row of [0, n)
__device__ __forceinline__ u64 bits_word(const u64* __restrict__ bits, int64_t wi, int64_t n) {
    const int64_t nw = (n + 63) >> 6;
    if (wi >= nw) return 0ull;
    u64 w = bits ? bits[wi] : ~0ull;
    const int tail = (int)(n & 63);
    if (wi == nw - 1 && tail) w &= (1ull << tail) - 1ull;
    return w;
}

// every thread of the workgroup: the popcounts of its words summed into *total with one device atomic
__device__ __forceinline__ void bits_count(int c, unsigned long long* total) {
    __shared__ int wtot[BW_NW];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    c = wave_sum_i(c);
    if (lane == 0) wtot[wid] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < BW_NW; ++i) t += wtot[i];
        if (t) atomicAdd(total, (unsigned long long)t);
    }
}

__global__ void __launch_bounds__(BW_THREADS) k_bits_fold(u64* __restrict__ acc, const u64* __restrict__ qbits, int nqb,
                                                          int64_t nwords) {
    const int64_t w = (int64_t)blockIdx.x * BW_THREADS + threadIdx.x;
    if (w >= nwords) return;
    u64 v = acc[w];
    for (int q = 0; q < nqb; ++q) v &= qbits[(int64_t)q * nwords + w];
    acc[w] = v;
}

__global__ void __launch_bounds__(BW_THREADS) k_bits_finish(const u64* __restrict__ acc, const u64* __restrict__ members,
                                                            int has_members, int64_t n_members, int negate,
                                                            int64_t n_sel, u64* __restrict__ out,
                                                            unsigned long long* total) {
    const int64_t nwords = (n_sel + 63) >> 6;
    const int64_t w = (int64_t)blockIdx.x * BW_THREADS + threadIdx.x;
    int c = 0;
    if (w < nwords) {
        const u64 m = has_members ? bits_word(members, w, n_members) : ~0ull;  // (n_members 0: no word is read)
        const u64 v = (negate ? ~acc[w] : acc[w]) & m & bits_word(nullptr, w, n_sel);
        out[w] = v;
        c = __popcll(v);
    }
    bits_count(c, total);
}

__global__ void __launch_bounds__(BW_THREADS) k_bits_op(const u64* __restrict__ a, int64_t na, const u64* __restrict__ b,
                                                        int64_t nb, int op, int64_t n_sel, u64* __restrict__ out,
                                                        unsigned long long* total) {
    const int64_t nwords = (n_sel + 63) >> 6;
    const int64_t w = (int64_t)blockIdx.x * BW_THREADS + threadIdx.x;
    int c = 0;
    if (w < nwords) {
        const u64 x = bits_word(a, w, na);
        const u64 y = op != VS_SEL_NOT ? bits_word(b, w, nb) : 0ull;  // (a null bitmap covers no row)
        u64 v = op == VS_SEL_AND ? x & y : op == VS_SEL_OR ? x | y : op == VS_SEL_ANDNOT ? x & ~y : ~x;
        v &= bits_word(nullptr, w, n_sel);
        out[w] = v;
        c = __popcll(v);
    }
    bits_count(c, total);
}

static bool bits_grid(int64_t nwords, unsigned* g) {
    const int64_t G = (nwords + BW_THREADS - 1) / BW_THREADS;
    if (nwords <= 0 || G > 0x7FFFFFFF) return false;
    *g = (unsigned)G;
    return true;
}

hipError_t launch_bits_fold(uint64_t* acc, const uint64_t* qbits, int nqb, int64_t nwords, hipStream_t st) {
    unsigned G;
    if (!acc || !qbits || nqb < 1 || !bits_grid(nwords, &G)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bits_fold, dim3(G), dim3(BW_THREADS), 0, st, (u64*)acc, (const u64*)qbits, nqb, nwords);
    return hipGetLastError();
}

hipError_t launch_bits_finish(const uint64_t* acc, bool has_members, const uint64_t* members, int64_t n_members,
                              int negate, int64_t n_sel, uint64_t* out, unsigned long long* total, hipStream_t st) {
    unsigned G;
    if (!acc || !out || !total || (has_members && (n_members < 0 || n_members > n_sel || (!members && n_members > 0))) ||
        !bits_grid((n_sel + 63) >> 6, &G))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bits_finish, dim3(G), dim3(BW_THREADS), 0, st, (const u64*)acc, (const u64*)members,
                       has_members ? 1 : 0, n_members, negate, n_sel, (u64*)out, total);
    return hipGetLastError();
}

hipError_t launch_bits_op(const uint64_t* a, int64_t na, const uint64_t* b, int64_t nb, int op, int64_t n_sel,
                          uint64_t* out, unsigned long long* total, hipStream_t st) {
    unsigned G;
    const bool unary = op == VS_SEL_NOT;
    if (na < 0 || na > n_sel || (!a && na > 0) || (!unary && (nb < 0 || nb > n_sel || (!b && nb > 0))) || !out || !total ||
        (op != VS_SEL_AND && op != VS_SEL_OR && op != VS_SEL_ANDNOT && op != VS_SEL_NOT) ||
        !bits_grid((n_sel + 63) >> 6, &G))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bits_op, dim3(G), dim3(BW_THREADS), 0, st, (const u64*)a, na, (const u64*)b, nb, op, n_sel,
                       (u64*)out, total);
    return hipGetLastError();
}

}  // namespace vs

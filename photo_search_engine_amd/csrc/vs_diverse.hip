// vs_diverse.hip -- the walk of the diversified search (include/vs.h "diversified search"; host:
// vs_diverse_host.hip).
//
// k_diverse_walk: one 256-thread workgroup per query goes through the query's exact ranking (a list of
// row ids, best first, of any length) and accepts a row iff it is near no row accepted before it --
// near: (float)S(a, b) passes the query's radius strictly, S the canonical fp64 score of the two
// stored rows (exact_score_rows with one of them staged in LDS as its fp64 query: the predicate of the
// range kernels, symmetric bit for bit) -- and otherwise counts it under the earliest-accepted row it
// is near.  The list is walked in blocks of DV_BLOCK candidates:
//   (a)  block x accepted: per candidate the lowest accepted index it is near
//   (b)  the block's survivors against each other: a DV_BLOCK x DV_BLOCK bit matrix in LDS
//   (c)  one thread resolves the block in order on those bits alone and appends to the accepted set
// (a) and (b) run in rounds: each wave stages one candidate row in its own LDS query slot (a.nqs
// slots: as many of the four as the dimension lets fit), a barrier, and the wave scores its candidate
// against the accepted rows (ascending, stopping at the first one it is near) or the earlier
// survivors, RR gathered rows per call.  A block in which (a) leaves no survivor skips (b).
// The accepted ids and their hidden counters live in LDS (k <= DV_K_MAX); rows never leave the device.
// Every store is bounded: the outputs by k entries of the query's rows, the LDS arrays by nk < k <=
// DV_K_MAX, by DV_BLOCK and by a.nqs slots of ng * 8 doubles.  Plain vector stores only.
#include "vs_device.h"
#include "vs_dispatch.h"

namespace vs {

static_assert(DV_BLOCK == 64, "k_diverse_walk: one ballot / one 64-bit word per block row");
constexpr int DV_NW = DV_THREADS / 64;
constexpr size_t DV_DYN_CAP = 112 * 1024;  // dynamic LDS beside ~29 KiB of static arrays

__device__ __forceinline__ bool dv_near(double S, float r, int metric) {
    const float D = (float)S;
    return metric == METRIC_IP ? D > r : D < r;
}

template <int DT, int METRIC>
__global__ void __launch_bounds__(DV_THREADS) k_diverse_walk(DiverseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [a.nqs][8 * ng] fp64 query slots
    constexpr int RR = refine_rows<DT>();
    constexpr int ES = DT == DT_F32 ? 4 : 2;
    constexpr int CE = CHB / ES;
    constexpr int NV = DT == DT_F32 ? 2 : 1;  // 16 B loads per unit of 8 elements
    constexpr int NONE = 0x7FFFFFFF;
    __shared__ uint32_t s_acc[DV_K_MAX];            // accepted row ids, acceptance order
    __shared__ int s_hid[DV_K_MAX];                 // rows hidden under each
    __shared__ int64_t s_cid[DV_BLOCK];             // the block's candidate ids (-1: past the list)
    __shared__ int s_near[DV_BLOCK];                // (a): lowest accepted index the candidate is near
    __shared__ int s_surv[DV_BLOCK];                // survivor -> position in the block
    __shared__ unsigned long long s_bits[DV_BLOCK]; // (b): survivor i is near survivors j < i (bit j)
    __shared__ int s_aidx[DV_BLOCK];                // (c): accepted index of an accepted survivor
    __shared__ int s_nb, s_ns, s_nk;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t* Iq = a.I_in + q * a.L;
    const float* Dq = a.D_in + q * a.L;
    int64_t* Io = a.I + q * a.k;
    float* Do = a.D + q * a.k;
    const float r = a.radius[q];
    const int ng = (a.d + 7) >> 3;
    const int nqs = a.nqs;
    double* qs = (double*)smem + (size_t)wid * 8 * ng;  // this wave's slot (wid < nqs)
    // stored row `row` as this wave's fp64 query, in exact_score_rows' [e * ng + g] order (16 B units
    // of 8 elements: a row's piece of a chunk is padded to whole units)
    auto stage_row = [&](int64_t row) {
        const uint8_t* rb = a.corpus + (row / TR) * (int64_t)TR * a.dpad * ES + (row % TR) * CHB;
        for (int g = lane; g < ng; g += 64) {
            const int i0 = 8 * g;
            const uint8_t* p = rb + (int64_t)(i0 / CE) * TR * CHB + (i0 % CE) * ES;
            float x[8];
#pragma unroll
            for (int v = 0; v < NV; ++v) unpack16<DT>(*(const uint4*)(p + 16 * v), x + 4 * v);
#pragma unroll
            for (int e = 0; e < 8; ++e) qs[e * ng + g] = (double)x[e];  // (elements past d are never read)
        }
    };
    int nk = 0;            // accepted so far (uniform)
    int64_t examined = 0;  // (thread 0's count)
    for (int64_t b0 = 0; b0 < a.L && nk < a.k; b0 += DV_BLOCK) {
        if (tid < DV_BLOCK) {
            int64_t id = b0 + tid < a.L ? Iq[b0 + tid] : -1;
            if (id < 0 || id >= a.n_valid) id = -1;
            s_cid[tid] = id;
            s_near[tid] = NONE;
            s_bits[tid] = 0ull;
            const u64 ok = __ballot(id >= 0);  // the list ends at its first absent entry
            if (tid == 0) s_nb = ~ok ? __ffsll((long long)~ok) - 1 : DV_BLOCK;
        }
        __syncthreads();
        const int nb = s_nb;
        if (nb == 0) break;
        // (a) block x accepted
        if (nk > 0) {
            for (int c0 = 0; c0 < nb; c0 += nqs) {
                const int c = c0 + wid;
                const bool mine = wid < nqs && c < nb;
                if (mine) stage_row(s_cid[c]);
                __syncthreads();
                if (mine) {
                    int lo = NONE;
                    for (int j0 = 0; j0 < nk && lo == NONE; j0 += RR) {
                        int64_t rr[RR];
#pragma unroll
                        for (int i = 0; i < RR; ++i) rr[i] = j0 + i < nk ? (int64_t)s_acc[j0 + i] : -1;
                        double s[RR];  // (the same in every lane: an xor butterfly)
                        exact_score_rows<DT, METRIC, true, RR>(a.corpus, rr, qs, nullptr, a.d, a.dpad, lane, s);
#pragma unroll
                        for (int i = RR - 1; i >= 0; --i)
                            if (j0 + i < nk && dv_near(s[i], r, METRIC)) lo = j0 + i;
                    }
                    if (lane == 0) s_near[c] = lo;
                }
                __syncthreads();  // (the slots are free again; s_near is published)
            }
        }
        if (tid < DV_BLOCK) {  // the survivors, in the block's order
            const bool sv = tid < nb && s_near[tid] == NONE;
            const u64 m = __ballot(sv);
            if (sv) s_surv[__popcll(m & ((1ull << tid) - 1ull))] = tid;
            if (tid == 0) s_ns = __popcll(m);
        }
        __syncthreads();
        const int ns = s_ns;
        // (b) survivors x earlier survivors
        for (int i0 = 1; i0 < ns; i0 += nqs) {
            const int i = i0 + wid;
            const bool mine = wid < nqs && i < ns;
            if (mine) stage_row(s_cid[s_surv[i]]);
            __syncthreads();
            if (mine) {
                unsigned long long bits = 0ull;
                for (int j0 = 0; j0 < i; j0 += RR) {
                    int64_t rr[RR];
#pragma unroll
                    for (int u = 0; u < RR; ++u) rr[u] = j0 + u < i ? s_cid[s_surv[j0 + u]] : -1;
                    double s[RR];
                    exact_score_rows<DT, METRIC, true, RR>(a.corpus, rr, qs, nullptr, a.d, a.dpad, lane, s);
#pragma unroll
                    for (int u = 0; u < RR; ++u)
                        if (j0 + u < i && dv_near(s[u], r, METRIC)) bits |= 1ull << (j0 + u);
                }
                if (lane == 0) s_bits[i] = bits;
            }
            __syncthreads();
        }
        // (c) the block in order, on bits alone
        if (tid == 0) {
            unsigned long long accm = 0ull;  // survivors accepted in this block
            int si = 0;
            for (int c = 0; c < nb; ++c) {
                ++examined;
                const int nr = s_near[c];
                if (nr != NONE) {
                    ++s_hid[nr];
                    continue;
                }
                const int i = si++;
                const unsigned long long m = s_bits[i] & accm;
                if (m) {
                    ++s_hid[s_aidx[__ffsll((long long)m) - 1]];  // (lower bit = accepted earlier)
                    continue;
                }
                s_acc[nk] = (uint32_t)s_cid[c];
                s_hid[nk] = 0;
                s_aidx[i] = nk;
                accm |= 1ull << i;
                Io[nk] = s_cid[c];
                Do[nk] = Dq[b0 + c];
                if (++nk == a.k) break;
            }
            s_nk = nk;
        }
        __syncthreads();
        nk = s_nk;
        if (nb < DV_BLOCK) break;
    }
    __syncthreads();
    for (int j = tid; j < a.k; j += DV_THREADS) {
        if (j >= nk) {
            Io[j] = -1;
            Do[j] = METRIC == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
        }
        a.hidden[q * a.k + j] = j < nk ? s_hid[j] : 0;
    }
    if (tid == 0) {
        a.nacc[q] = nk;
        a.examined[q] = examined;
    }
}

int diverse_query_slots(int d) {
    return (int)std::min<size_t>(DV_NW, DV_DYN_CAP / query_lds_bytes(d));
}

hipError_t launch_diverse_walk(const DiverseArgs& a, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (a.k < 1 || a.k > DV_K_MAX || a.L < 1 || a.d < 1 || a.n_valid > 0xFFFFFFFFll || !a.corpus || !a.I_in || !a.D_in ||
        !a.radius || !a.I || !a.D || !a.hidden || !a.nacc || !a.examined ||
        (a.metric != METRIC_IP && a.metric != METRIC_L2) || a.nqs < 1 || a.nqs != diverse_query_slots(a.d))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)a.nqs * query_lds_bytes(a.d);
    const bool known = dispatch(a.dt, a.metric, [&](auto dt, auto metric) {
        launch_kernel(k_diverse_walk<dt, metric>, (int)DV_DYN_CAP, dim3(nq), dim3(DV_THREADS), lds, st, a);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

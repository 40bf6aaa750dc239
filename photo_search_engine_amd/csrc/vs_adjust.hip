// vs_adjust.hip -- the kernels of the adjusted search (include/vs.h "adjusted search"; host:
// vs_adjust_host.hip).
//
// A row's adjusted score is A = fl64(fl64((double)scale * S) + (double)bias): two rounded fp64
// operations (__dmul_rn / __dadd_rn: never contracted into an FMA) on the canonical fp64 score S.
//
// k_adjust_scan: fs_scan_body (vs_scan.h) with a transform -- the running top-k is kept under A instead
// of S.  Over an id list (the adjusted rows of a vs_adjust, or a selector's rows) or over rows
// [0, n_cov); rows the caller's selector does not allow, and rows behind the covered ones, are passed
// over.  Either sequence ascends in id, so the scan's tie argument holds unchanged under A.
//
// k_adjust_walk: one workgroup per query ranks up to AJ_N_MAX entries -- a prefix of the query's exact
// plain ranking (row ids only: the staged fp32 scores are never used) and, behind it, the query's
// adjusted-scan list -- by (A, id).  Every entry is rescored canonically (exact_score_rows, the query as
// fp64 in LDS, RR entries per wave at a time); lane 0 gathers the entry's (scale, bias), forms A and
// puts (key, id) into LDS, key = A or -A for L2, and S into the query's scratch row.  The entries are
// sorted best first (sort_valid_best_first), then every entry finds its own rank by binary search and,
// if it is below k, writes its A, S and id there -- S never has to travel through the sort.  What the
// answer is worth depends on the mode (AdjustWalkArgs::mode): the proofs are in DESIGN §7j.
// Every store is bounded: LDS by n2 >= L + ks entries, the scratch row by L + ks, the outputs by rank <
// k; a list entry at or past n_cov ends the list like an absent one.  Plain vector stores only.
#include "vs_scan.h"

namespace vs {

__device__ __forceinline__ double adjust_score(float scale, float bias, double S) {
    return __dadd_rn(__dmul_rn((double)scale, S), (double)bias);
}
__device__ __forceinline__ bool adjust_plain(float scale, float bias) { return scale == 1.0f && bias == 0.0f; }

struct AdjustXf {
    static constexpr bool active = true;
    AdjustRows r;
    template <int METRIC>
    __device__ __forceinline__ bool key(uint32_t id, double S, double& s) const {
        if ((int64_t)id >= r.n_cov) return false;
        if (r.sel_bits && !((int64_t)id < r.n_sel && ((r.sel_bits[id >> 6] >> (id & 63)) & 1ull))) return false;
        const double A = adjust_score(r.scale[id], r.bias[id], S);
        s = METRIC == METRIC_L2 ? -A : A;
        return true;
    }
};

template <int DT, int METRIC, bool QLDS, bool SEL>
__global__ void __launch_bounds__(FS_THREADS) k_adjust_scan(FullScanArgs a, int KL, AdjustRows r,
                                                            const uint32_t* __restrict__ ids, int64_t m) {
    fs_scan_body<DT, METRIC, QLDS, SEL, AdjustXf>(a, KL, ids, m, AdjustXf{r});
}

hipError_t launch_adjust_scan(const FullScanArgs& a, const AdjustRows& r, const uint32_t* ids, int64_t m, int qy,
                              hipStream_t st) {
    if (qy < 1 || qy > a.nq || qy > 65535 || !r.scale || !r.bias || r.n_cov <= 0 || (!ids && a.n_valid != r.n_cov) ||
        (ids && m <= 0))
        return hipErrorInvalidValue;
    return fs_launch_scan(
        a, 1, ids != nullptr, ids ? qy : 1, st,
        [](auto dt, auto metric, auto qlds, auto sel) { return k_adjust_scan<dt, metric, qlds, sel>; }, r, ids, m);
}

// ---- the walk ------------------------------------------------------------------------------------
constexpr int AJ_NW = AJ_THREADS / 64;

template <int DT, int METRIC>
__global__ void __launch_bounds__(AJ_THREADS) k_adjust_walk(AdjustWalkArgs a, int n2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [key fp64 n2 | query fp64 8 ng | id n2]
    constexpr int RR = refine_rows<DT>();
    __shared__ int s_nL, s_nS, s_np, s_nd;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ng = (a.d + 7) >> 3;
    double* key = (double*)smem;
    double* qs = key + n2;
    uint32_t* eid = (uint32_t*)(qs + (size_t)8 * ng);
    const int L = a.I_list ? (int)a.L : 0, ks = a.I_scan ? a.ks : 0;
    const int64_t* Il = a.I_list ? a.I_list + q * a.L : nullptr;
    const int64_t* Is = a.I_scan ? a.I_scan + (a.qmap ? a.qmap[q] : q) * a.ks : nullptr;
    double* St = a.S_tmp + q * (int64_t)(L + ks);
    const float* qv = a.q + q * a.d;
    int64_t* Io = a.I + q * a.k;
    float* Do = a.D + q * a.k;
    float* Ro = a.D_raw + q * a.k;
    if (tid == 0) {
        s_nL = L;
        s_nS = ks;
        s_np = 0;
        s_nd = 0;
    }
    __syncthreads();
    // either list ends at its first absent entry (an id at or past n_cov is no member: it ends it too)
    for (int i = tid; i < L; i += AJ_THREADS) {
        const int64_t id = Il[i];
        if (id < 0 || id >= a.rows.n_cov) atomicMin(&s_nL, i);
    }
    for (int i = tid; i < ks; i += AJ_THREADS) {
        const int64_t id = Is[i];
        if (id < 0 || id >= a.rows.n_cov) atomicMin(&s_nS, i);
    }
    for (int i = tid; i < a.d; i += AJ_THREADS) qs[(i & 7) * ng + (i >> 3)] = (double)qv[i];
    __syncthreads();
    const int nL = s_nL, nS = s_nS, N = nL + nS;  // N <= L + ks <= n2
    auto entry = [&](int p) -> int64_t { return p < nL ? Il[p] : Is[p - nL]; };
    for (int base = 0; base < N; base += AJ_NW * RR) {
        int64_t rr[RR];
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int p = base + wid + i * AJ_NW;
            rr[i] = p < N ? entry(p) : -1;
        }
        if (rr[0] < 0) continue;  // (wave-uniform; later entries of the wave are absent too)
        double s[RR];
        exact_score_rows<DT, METRIC, true, RR>(a.corpus, rr, qs, nullptr, a.d, a.dpad, lane, s);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < RR; ++i) {
                if (rr[i] < 0) continue;
                const int p = base + wid + i * AJ_NW;
                const float sc = a.rows.scale[rr[i]], bi = a.rows.bias[rr[i]];
                const bool plain = adjust_plain(sc, bi);
                const bool drop = a.mode == AJ_DIRECT && p < nL && !plain;
                const double A = adjust_score(sc, bi, s[i]);
                key[p] = drop ? -INFINITY : (METRIC == METRIC_L2 ? -A : A);
                eid[p] = drop ? 0xFFFFFFFFu : (uint32_t)rr[i];
                St[p] = s[i];
                if (drop) atomicAdd(&s_nd, 1);
                else if (p < nL && plain) atomicAdd(&s_np, 1);
            }
        }
    }
    for (int j = N + tid; j < n2; j += AJ_THREADS) {
        key[j] = -INFINITY;
        eid[j] = 0xFFFFFFFFu;
    }
    __syncthreads();
    if (N > 0) sort_valid_best_first<METRIC_IP>(key, eid, N, n2);  // (dropped entries sort behind every kept one)
    const int nv = N - s_nd;
    for (int p = tid; p < N; p += AJ_THREADS) {
        const int64_t id = entry(p);
        const float sc = a.rows.scale[id], bi = a.rows.bias[id];
        if (a.mode == AJ_DIRECT && p < nL && !adjust_plain(sc, bi)) continue;
        const double S = St[p];
        const double A = adjust_score(sc, bi, S);
        const int r = fs_rank(key, eid, nv, METRIC == METRIC_L2 ? -A : A, (uint32_t)id);
        if (r < a.k) {
            Io[r] = id;
            Do[r] = (float)A;
            Ro[r] = (float)S;
        }
    }
    const float worst = METRIC == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
    for (int j = nv + tid; j < a.k; j += AJ_THREADS) {
        Io[j] = -1;
        Do[j] = worst;
        Ro[j] = worst;
    }
    if (tid == 0) {
        bool done;
        if (a.mode == AJ_PLAIN || nL < L) {
            done = true;
        } else if (a.mode == AJ_DIRECT) {
            done = s_np >= a.k;
        } else if (nv < a.k || nL < 1) {
            done = false;
        } else {
            // every member behind the list has S <= S_L (L2: >=), scale >= 0 and the rounded multiply and add
            // are monotone: its A is at most U (L2: at least)
            const double SL = St[nL - 1];
            if (METRIC == METRIC_IP) {
                const double u0 = __dadd_rn(__dmul_rn(a.smax, SL), a.bmax), u1 = __dadd_rn(__dmul_rn(a.smin, SL), a.bmax);
                done = key[a.k - 1] > (u0 > u1 ? u0 : u1);
            } else {
                const double u0 = __dadd_rn(__dmul_rn(a.smin, SL), a.bmin), u1 = __dadd_rn(__dmul_rn(a.smax, SL), a.bmin);
                done = -key[a.k - 1] < (u0 < u1 ? u0 : u1);
            }
        }
        a.complete[q] = done ? 1 : 0;
    }
}

size_t adjust_walk_lds(int64_t n_entries, int d) { return pow2_at_least(n_entries, 64) * 12 + query_lds_bytes(d); }

hipError_t launch_adjust_walk(const AdjustWalkArgs& a, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    const int64_t n = (a.I_list ? a.L : 0) + (a.I_scan ? a.ks : 0);
    if (a.k < 1 || a.k > K_MAX || n < 1 || n > AJ_N_MAX || (a.I_list && a.L < 1) || (a.I_scan && a.ks < 1) || a.d < 1 ||
        !a.corpus || !a.q || !a.rows.scale || !a.rows.bias || a.rows.n_cov < 1 || a.rows.n_cov > 0xFFFFFFFFll || !a.S_tmp ||
        !a.I || !a.D || !a.D_raw || !a.complete || (a.metric != METRIC_IP && a.metric != METRIC_L2) ||
        (a.mode != AJ_PLAIN && a.mode != AJ_DIRECT && a.mode != AJ_BOUND) || (a.mode != AJ_PLAIN && !a.I_list) ||
        (a.mode == AJ_BOUND && a.I_scan))
        return hipErrorInvalidValue;
    const size_t lds = adjust_walk_lds(n, a.d);
    if (lds > AJ_DYN_CAP) return hipErrorInvalidValue;
    const int n2 = (int)pow2_at_least(n, 64);
    const bool known = dispatch(a.dt, a.metric, [&](auto dt, auto metric) {
        launch_kernel(k_adjust_walk<dt, metric>, (int)AJ_DYN_CAP, dim3(nq), dim3(AJ_THREADS), lds, st, a, n2);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

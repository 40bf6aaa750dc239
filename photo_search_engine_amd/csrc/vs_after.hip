// vs_after.hip -- the kernels of the paged search (include/vs.h "paged search"; host: vs_after_host.hip;
// DESIGN §7l).
//
// A query's cursor is the position (S*, c) in vs_search's total order, c a stored row and S* its canonical
// fp64 score with the query; the answer is the members strictly after it.  Inside the kernels a score is
// held as its key, S or -S for L2, so "better" is always "greater", and the one comparison of the whole
// job is fs_better (vs_scan.h): numeric on doubles (+0.0 and -0.0 tie), then the lower id.  A row (s, id)
// is strictly after the cursor iff fs_better(S*, c, s, id).
//
// k_after_score: one wave per query scores row after[q] canonically (exact_score_rows, the query read
// from global memory: the same expression tree as with the query in LDS) and writes its key.  after[q] =
// -1 stays the flag "from the top" in the id array itself.
//
// k_after_cut: one workgroup per query cuts a prefix of the query's exact ranking among the members (row
// ids and the staged fp32 scores D = (float)S) at the cursor.  Rounding to fp32 is monotone: S_a better
// than S_b implies (float)S_a at least as good as (float)S_b.  So an entry whose D is strictly better
// (worse) than (float)S* has S strictly better (worse) than S*: it is before (after) the cursor, whatever
// its id.  The entries with D == (float)S* -- one run of the list, since D is monotone along it -- decide
// nothing by D: two distinct S can round to one D and the cursor can sit inside such a run, so each of
// them is rescored canonically (the query as fp64 in LDS, RR entries per wave at a time) and compared by
// (S, id).  p = the entries at or before the cursor; the page is entries p .. p + k - 1 as staged.
// Every store is bounded: LDS by the query's 8 ng doubles, the outputs by j < k; a list entry at or past
// n_valid ends the list like an absent one.  Plain vector stores only.
//
// k_after_scan: fs_scan_body (vs_scan.h) with a per-query transform -- every row of the sequence at or
// before the query's cursor is passed over and counted; the workgroup adds its count to rank[q] with one
// device atomic per query.  Over rows [0, n) or a selector's id list: both sequences ascend in id, so the
// scan's tie argument ("a row tied with the k-th best never enters a full list") holds among the rows
// after the cursor, the only ones that reach the lists.
#include "vs_scan.h"

namespace vs {

// ---- cursor scoring ------------------------------------------------------------------------------
template <int DT, int METRIC>
__global__ void __launch_bounds__(64) k_after_score(const uint8_t* __restrict__ corpus, int d, int dpad, int64_t n_valid,
                                                    const float* __restrict__ q, const int64_t* __restrict__ after,
                                                    double* __restrict__ key) {
    const int64_t qi = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t c = after[qi];
    if (c < 0 || c >= n_valid) {  // (block-uniform) from the top; the host admits no id at or past n_valid
        if (lane == 0) key[qi] = 0.0;
        return;
    }
    const int64_t rr[1] = {c};
    double s[1];
    exact_score_rows<DT, METRIC, false, 1>(corpus, rr, nullptr, q + qi * d, d, dpad, lane, s);
    if (lane == 0) key[qi] = METRIC == METRIC_L2 ? -s[0] : s[0];
}

hipError_t launch_after_score(int dt, int metric, const uint8_t* corpus, int d, int dpad, int64_t n_valid, const float* q,
                              const int64_t* after, int64_t nq, double* key, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (!corpus || !q || !after || !key || d < 1 || n_valid < 0 || (metric != METRIC_IP && metric != METRIC_L2))
        return hipErrorInvalidValue;
    const int64_t qmax = 65536;  // workgroups of one launch
    bool known = true;
    for (int64_t q0 = 0; q0 < nq && known; q0 += qmax) {
        const int n = (int)std::min(qmax, nq - q0);
        known = dispatch(dt, metric, [&](auto dt_c, auto metric_c) {
            launch_kernel(k_after_score<dt_c, metric_c>, 0, dim3(n), dim3(64), 0, st, corpus, d, dpad, n_valid, q + q0 * d,
                          after + q0, key + q0);
        });
    }
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

// ---- the cut -------------------------------------------------------------------------------------
constexpr int AF_NW = AF_THREADS / 64;

template <int DT, int METRIC>
__global__ void __launch_bounds__(AF_THREADS) k_after_cut(AfterCutArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [query fp64 8 ng]
    constexpr int RR = refine_rows<DT>();
    __shared__ int s_nL, s_nb, s_ne, s_pe;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ng = (a.d + 7) >> 3;
    double* qs = (double*)smem;
    const int L = (int)a.L;
    const int64_t* Il = a.I_list + q * a.L;
    const float* Dl = a.D_list + q * a.L;
    const int64_t cq = a.cur.qmap ? a.cur.qmap[q] : q;
    const int64_t c = a.cur.id[cq];
    const double ck = c >= 0 ? a.cur.key[cq] : 0.0;
    int64_t* Io = a.I + q * a.k;
    float* Do = a.D + q * a.k;
    if (tid == 0) {
        s_nL = L;
        s_nb = 0;
        s_ne = 0;
        s_pe = 0;
    }
    __syncthreads();
    // the list ends at its first absent entry (an id at or past n_valid is no row: it ends it too)
    for (int i = tid; i < L; i += AF_THREADS) {
        const int64_t id = Il[i];
        if (id < 0 || id >= a.n_valid) atomicMin(&s_nL, i);
    }
    __syncthreads();
    const int nL = s_nL;
    int p = 0;
    if (c >= 0) {  // (block-uniform)
        // the cursor's own D, in the metric's direction as the list holds it ((float)-x == -(float)x)
        const float fc = (float)(METRIC == METRIC_L2 ? -ck : ck);
        int nb = 0, ne = 0;
        for (int i = tid; i < nL; i += AF_THREADS) {
            const float Di = Dl[i];
            if (METRIC == METRIC_L2 ? Di < fc : Di > fc) ++nb;
            else if (Di == fc) ++ne;
        }
        if (nb) atomicAdd(&s_nb, nb);
        if (ne) atomicAdd(&s_ne, ne);
        __syncthreads();
        const int b0 = s_nb, b1 = b0 + s_ne;  // D is monotone along the list: the run with D == fc is [b0, b1)
        if (b1 > b0) {  // (block-uniform)
            for (int i = tid; i < a.d; i += AF_THREADS) qs[(i & 7) * ng + (i >> 3)] = (double)a.q[q * a.d + i];
            __syncthreads();
            for (int base = b0; base < b1; base += AF_NW * RR) {
                int64_t rr[RR];
#pragma unroll
                for (int i = 0; i < RR; ++i) {
                    const int e = base + wid + i * AF_NW;
                    rr[i] = e < b1 ? Il[e] : -1;
                }
                if (rr[0] < 0) continue;  // (wave-uniform; later entries of the wave are absent too)
                double s[RR];
                exact_score_rows<DT, METRIC, true, RR>(a.corpus, rr, qs, nullptr, a.d, a.dpad, lane, s);
                if (lane == 0) {
                    int cnt = 0;
#pragma unroll
                    for (int i = 0; i < RR; ++i) {
                        if (rr[i] < 0) continue;
                        const double si = METRIC == METRIC_L2 ? -s[i] : s[i];
                        if (!fs_better(ck, (uint32_t)c, si, (uint32_t)rr[i])) ++cnt;  // at or before the cursor
                    }
                    if (cnt) atomicAdd(&s_pe, cnt);
                }
            }
            __syncthreads();
        }
        p = b0 + s_pe;
    }
    const float worst = METRIC == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
    for (int j = tid; j < a.k; j += AF_THREADS) {
        const int e = p + j;
        Io[j] = e < nL ? Il[e] : -1;
        Do[j] = e < nL ? Dl[e] : worst;
    }
    if (tid == 0) {
        a.rank[q] = p;
        a.complete[q] = (nL - p >= a.k || nL < L) ? 1 : 0;
    }
}

hipError_t launch_after_cut(const AfterCutArgs& a, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (nq > 65536 || a.k < 1 || a.k > K_MAX || a.L < 1 || a.L > K_MAX || a.d < 1 || a.d > AF_D_MAX || !a.corpus || !a.q ||
        !a.I_list || !a.D_list || a.n_valid < 1 || a.n_valid > 0xFFFFFFFFll || !a.cur.id || !a.cur.key || !a.I || !a.D ||
        !a.rank || !a.complete || (a.metric != METRIC_IP && a.metric != METRIC_L2))
        return hipErrorInvalidValue;
    const bool known = dispatch(a.dt, a.metric, [&](auto dt, auto metric) {
        launch_kernel(k_after_cut<dt, metric>, (int)query_lds_bytes(AF_D_MAX), dim3(nq), dim3(AF_THREADS),
                      query_lds_bytes(a.d), st, a);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

// ---- the scan ------------------------------------------------------------------------------------
// fs_scan_body's paged transform: the rows at or before query q's cursor are passed over and counted
struct AfterXf {
    static constexpr bool active = true;
    static constexpr bool per_query = true;
    AfterCursor cur;
    unsigned long long* rank;
    template <int METRIC>
    __device__ __forceinline__ bool key(int q, uint32_t id, double s, unsigned& passed) const {
        const int64_t cq = cur.qmap ? cur.qmap[q] : q;
        const int64_t c = cur.id[cq];
        if (c < 0) return true;
        if (fs_better(cur.key[cq], (uint32_t)c, s, id)) return true;
        ++passed;
        return false;
    }
    __device__ __forceinline__ void count(int q, unsigned n) const { atomicAdd(rank + q, (unsigned long long)n); }
};

template <int DT, int METRIC, bool QLDS, bool SEL>
__global__ void __launch_bounds__(FS_THREADS) k_after_scan(FullScanArgs a, int KL, AfterCursor cur, unsigned long long* rank,
                                                           const uint32_t* __restrict__ ids, int64_t m) {
    fs_scan_body<DT, METRIC, QLDS, SEL, AfterXf>(a, KL, ids, m, AfterXf{cur, rank});
}

hipError_t launch_after_scan(const FullScanArgs& a, const AfterCursor& cur, unsigned long long* rank, const uint32_t* ids,
                             int64_t m, int qy, hipStream_t st) {
    if (qy < 1 || qy > a.nq || qy > 65535 || a.n_valid > 0xFFFFFFFFll || a.gate || !a.all_queries || !cur.id || !cur.key ||
        !rank || (ids && m <= 0))
        return hipErrorInvalidValue;
    return fs_launch_scan(
        a, 1, ids != nullptr, ids ? qy : 1, st,
        [](auto dt, auto metric, auto qlds, auto sel) { return k_after_scan<dt, metric, qlds, sel>; }, cur, rank, ids, m);
}

}  // namespace vs

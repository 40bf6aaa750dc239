// vs_fuse.hip -- the kernels of the fused search (include/vs.h "fused search"; host: vs_fuse_host.hip;
// DESIGN §7k).
//
// A fused query is m sub-queries (1..FUSE_MAX_Q).  A row's fused score F is the best (ANY) or the worst
// (ALL) of its m canonical fp64 scores S_0..S_{m-1}: a selection, never arithmetic, so F is bit-equal to
// one of them; `which` is the lowest j with S_j == F.  Inside the kernels a score is held as its key,
// S or -S for L2, so "better" is always "greater" (fs_better).
//
// k_fuse_scan: fs_scan_body (vs_scan.h) with a fused transform -- the running top-k is kept under F.
// Every row of the workgroup's share is scored against all m sub-queries in one pass over its elements
// (fuse_score_rows: the row's registers are used m times, each (row, j) accumulator in the order of
// exact_score_rows, so every S_j is the canonical score bit for bit); the sub-queries are held as fp64 in
// LDS where they fit beside the lists, else read from global memory.  (F, id) goes through the bounded
// running top-k and the last workgroup's merge unchanged: both sequences ascend in id and F is a function
// of the row, so the scan's tie argument holds.
//
// k_fuse_walk: one workgroup per fused query ranks up to FUSE_WALK_MAX entries -- nl lists of L row ids
// (the m sub-queries' exact rankings, or the scan's one list; the staged fp32 scores are never used) --
// by (F, id).  The ids are sorted (the bitonic network under a constant key), duplicates are struck out
// and the N distinct ones packed to the front by a second sort; they go to the scratch row E_tmp.  Then,
// one sub-query at a time as fp64 in LDS, every distinct entry is rescored canonically
// (exact_score_rows, RR entries per wave at a time) into S_tmp [N][m].  Every entry forms its F, the
// (F, id) pairs are sorted best first, and every entry finds its own rank by binary search and, if it is
// below k, writes its id, F, which and its m scores there.  The ALL certificate is in DESIGN §7k.
// Every store is bounded: LDS by n2 >= nl L entries, the scratch rows by N <= nl L, the outputs by rank <
// k; an entry at or past n_valid ends its list like an absent one.  Plain vector stores only.
#include "vs_fuse_score.h"
#include "vs_scan.h"

namespace vs {

// the fused key of keys kj[0, m) (greater = better) and the lowest index that holds it
__device__ __forceinline__ void fuse_pick(int mode, int j, double kj, double& f, int& w) {
    if (j == 0 || (mode == FUSE_ANY ? kj > f : kj < f)) {
        f = kj;
        w = j;
    }
}

// ---- the scan ------------------------------------------------------------------------------------
// fs_scan_body's fused transform: m sub-queries per query, the row's F (in the metric's own direction) to
// the running top-k
struct FuseXf {
    static constexpr bool active = false;
    static constexpr bool fused = true;
    int m, mode;
    // qv [m][d] fp32 -> qs [m][8][ng] fp64
    __device__ __forceinline__ void load_queries(double* qs, const float* qv, int d, int ng, int tid) const {
        for (int i = tid; i < m * d; i += FS_THREADS) {
            const int j = i / d, e = i - j * d;
            qs[((size_t)j * 8 + (e & 7)) * ng + (e >> 3)] = (double)qv[i];
        }
    }
    template <int DT, int METRIC, bool QLDS, int R>
    __device__ __forceinline__ void score_rows(const FullScanArgs& a, const int64_t (&rr)[R], const double* qs,
                                               const float* qv, int lane, double (&F)[R]) const {
        double sj[FUSE_MAX_Q][R];
        fuse_score_rows<DT, METRIC, QLDS, R>(a.corpus, rr, qs, qv, m, a.d, a.dpad, lane, sj);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            double f = 0.0;
            int w = 0;
#pragma unroll
            for (int j = 0; j < FUSE_MAX_Q; ++j)
                if (j < m) fuse_pick(mode, j, METRIC == METRIC_L2 ? -sj[j][i] : sj[j][i], f, w);
            F[i] = METRIC == METRIC_L2 ? -f : f;
        }
    }
};

template <int DT, int METRIC, bool QLDS, bool SEL>
__global__ void __launch_bounds__(FS_THREADS) k_fuse_scan(FullScanArgs a, int KL, int m, int mode,
                                                          const uint32_t* __restrict__ sel_ids, int64_t sel_m) {
    fs_scan_body<DT, METRIC, QLDS, SEL, FuseXf>(a, KL, sel_ids, sel_m, FuseXf{m, mode});
}

hipError_t launch_fuse_scan(const FullScanArgs& a, int m, int mode, const uint32_t* ids, int64_t n_ids, int qy,
                            hipStream_t st) {
    if (qy < 1 || qy > a.nq || qy > 65535 || m < 1 || m > FUSE_MAX_Q || (mode != FUSE_ANY && mode != FUSE_ALL) ||
        a.n_valid > 0xFFFFFFFFll || a.gate || !a.all_queries || (ids && n_ids <= 0))
        return hipErrorInvalidValue;
    return fs_launch_scan(
        a, m, ids != nullptr, qy, st,
        [](auto dt, auto metric, auto qlds, auto sel) { return k_fuse_scan<dt, metric, qlds, sel>; }, m, mode, ids, n_ids);
}

// ---- the walk ------------------------------------------------------------------------------------
constexpr int FU_THREADS = 512;  // k_fuse_walk: one workgroup per fused query
constexpr int FU_NW = FU_THREADS / 64;
static_assert(FUSE_WALK_MAX <= 32 * FU_THREADS, "the duplicate mask keeps one bit per entry of a thread");

template <int DT, int METRIC>
__global__ void __launch_bounds__(FU_THREADS) k_fuse_walk(FuseWalkArgs a, int n2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [key fp64 n2 | one sub-query fp64 8 ng | id n2]
    constexpr int RR = refine_rows<DT>();
    __shared__ int s_len[FUSE_MAX_Q];
    __shared__ double s_u[FUSE_MAX_Q];
    __shared__ int s_n, s_dup;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ng = (a.d + 7) >> 3;
    double* key = (double*)smem;
    double* qs = key + n2;
    uint32_t* eid = (uint32_t*)(qs + (size_t)8 * ng);
    const int m = a.m, nl = a.nl, L = (int)a.L, NE = nl * L;  // NE <= n2
    const int64_t* Il = a.I_list + q * (int64_t)NE;
    double* St = a.S_tmp + q * (int64_t)NE * m;
    uint32_t* Et = a.E_tmp + q * (int64_t)NE;
    int64_t* Io = a.I + q * a.k;
    float* Do = a.D + q * a.k;
    int32_t* Wo = a.which + q * a.k;
    float* Uo = a.D_sub ? a.D_sub + q * (int64_t)a.k * m : nullptr;
    if (tid < FUSE_MAX_Q) s_len[tid] = L;
    if (tid == 0) {
        s_n = 0;
        s_dup = 0;
    }
    __syncthreads();
    // a list ends at its first absent entry (an id at or past n_valid is no row: it ends it too)
    for (int p = tid; p < NE; p += FU_THREADS) {
        const int64_t id = Il[p];
        if (id < 0 || id >= a.n_valid) atomicMin(&s_len[p / L], p % L);
    }
    __syncthreads();
    for (int p = tid; p < n2; p += FU_THREADS) {
        const bool in = p < NE && p % L < s_len[p / L];
        key[p] = in ? 0.0 : -INFINITY;
        eid[p] = in ? (uint32_t)Il[p] : 0xFFFFFFFFu;
    }
    __syncthreads();
    // the ids ascending (one key, so the order is the id's), the absent ones behind; then every repeat of
    // an id is struck out and a second sort packs the distinct ones to the front
    sort_best_first<METRIC_IP>(key, eid, n2);
    __syncthreads();
    {
        uint32_t dup = 0u;
        int cnt = 0;
        for (int p = tid, i = 0; p < n2; p += FU_THREADS, ++i) {
            const uint32_t id = eid[p];
            if (id == 0xFFFFFFFFu) continue;
            if (p > 0 && eid[p - 1] == id) dup |= 1u << i;
            else ++cnt;
        }
        __syncthreads();  // (every neighbour is read before any entry is struck out)
        for (int p = tid, i = 0; p < n2; p += FU_THREADS, ++i)
            if ((dup >> i) & 1u) {
                key[p] = -INFINITY;
                eid[p] = 0xFFFFFFFFu;
            }
        if (cnt) atomicAdd(&s_n, cnt);
        if (dup) atomicOr(&s_dup, 1);
    }
    __syncthreads();
    if (s_dup) {  // (block-uniform)
        sort_best_first<METRIC_IP>(key, eid, n2);
        __syncthreads();
    }
    const int N = s_n;  // distinct entries, <= NE
    for (int p = tid; p < N; p += FU_THREADS) Et[p] = eid[p];
    // every distinct entry against every sub-query, one sub-query in LDS at a time
    for (int j = 0; j < m; ++j) {
        __syncthreads();  // (the previous sub-query's readers of qs are done)
        const float* qv = a.q + (q * m + j) * a.d;
        for (int i = tid; i < a.d; i += FU_THREADS) qs[(i & 7) * ng + (i >> 3)] = (double)qv[i];
        __syncthreads();
        for (int base = 0; base < N; base += FU_NW * RR) {
            int64_t rr[RR];
#pragma unroll
            for (int i = 0; i < RR; ++i) {
                const int p = base + wid + i * FU_NW;
                rr[i] = p < N ? (int64_t)eid[p] : -1;
            }
            if (rr[0] < 0) continue;  // (wave-uniform; later entries of the wave are absent too)
            double s[RR];
            exact_score_rows<DT, METRIC, true, RR>(a.corpus, rr, qs, nullptr, a.d, a.dpad, lane, s);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < RR; ++i)
                    if (rr[i] >= 0) St[(size_t)(base + wid + i * FU_NW) * m + j] = s[i];
            }
        }
    }
    __syncthreads();
    auto fused = [&](int p, double& f, int& w) {
        for (int j = 0; j < m; ++j) {
            const double s = St[(size_t)p * m + j];
            fuse_pick(a.mode, j, METRIC == METRIC_L2 ? -s : s, f, w);
        }
    };
    for (int p = tid; p < N; p += FU_THREADS) {
        double f = 0.0;
        int w = 0;
        fused(p, f, w);
        key[p] = f;
    }
    __syncthreads();
    if (N > 0) sort_valid_best_first<METRIC_IP>(key, eid, N, n2);
    __syncthreads();
    for (int p = tid; p < N; p += FU_THREADS) {
        const uint32_t id = Et[p];
        double f = 0.0;
        int w = 0;
        fused(p, f, w);
        const int r = fs_rank(key, eid, N, f, id);
        if (r < a.k) {
            Io[r] = (int64_t)id;
            Do[r] = (float)(METRIC == METRIC_L2 ? -f : f);
            Wo[r] = w;
            if (Uo)
                for (int j = 0; j < m; ++j) Uo[(size_t)r * m + j] = (float)St[(size_t)p * m + j];
        }
    }
    const float worst = METRIC == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
    for (int r = N + tid; r < a.k; r += FU_THREADS) {
        Io[r] = -1;
        Do[r] = worst;
        Wo[r] = -1;
        if (Uo)
            for (int j = 0; j < m; ++j) Uo[(size_t)r * m + j] = worst;
    }
    // ALL's certificate: a member outside every list is, for every j, no better than list j's last entry
    // under sub-query j, so its F is no better than U, the worst of those m scores (the walk's own)
    bool open = false;  // (block-uniform) every list full: the bound decides
    if (a.certify) {
        open = true;
        for (int j = 0; j < nl; ++j) open = open && s_len[j] == L;
    }
    if (open && N >= a.k && tid < nl) {
        const uint32_t id = (uint32_t)Il[tid * L + L - 1];
        int lo = 0, hi = N - 1;  // (the id is among the N distinct ones)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (Et[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        const double s = St[(size_t)lo * m + tid];
        s_u[tid] = METRIC == METRIC_L2 ? -s : s;
    }
    __syncthreads();
    if (tid == 0) {
        bool done = true;
        if (open) {
            done = false;
            if (N >= a.k) {
                double u = s_u[0];
                for (int j = 1; j < nl; ++j) u = s_u[j] < u ? s_u[j] : u;
                done = key[a.k - 1] > u;
            }
        }
        a.complete[q] = done ? 1 : 0;
    }
}

size_t fuse_walk_lds(int64_t n_entries, int d) { return pow2_at_least(n_entries, 64) * 12 + query_lds_bytes(d); }

hipError_t launch_fuse_walk(const FuseWalkArgs& a, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    const int64_t n = (int64_t)a.nl * a.L;
    if (a.k < 1 || a.k > FUSE_WALK_MAX || a.m < 1 || a.m > FUSE_MAX_Q || (a.nl != 1 && a.nl != a.m) || a.L < 1 ||
        n > FUSE_WALK_MAX || a.d < 1 || !a.corpus || !a.q || !a.I_list || a.n_valid < 1 || a.n_valid > 0xFFFFFFFFll ||
        !a.S_tmp || !a.E_tmp || !a.I || !a.D || !a.which || !a.complete || (a.metric != METRIC_IP && a.metric != METRIC_L2) ||
        (a.mode != FUSE_ANY && a.mode != FUSE_ALL) || (a.certify && a.nl != a.m))
        return hipErrorInvalidValue;
    const size_t lds = fuse_walk_lds(n, a.d);
    if (lds > FUSE_DYN_CAP) return hipErrorInvalidValue;
    const int n2 = (int)pow2_at_least(n, 64);
    const bool known = dispatch(a.dt, a.metric, [&](auto dt, auto metric) {
        launch_kernel(k_fuse_walk<dt, metric>, (int)FUSE_DYN_CAP, dim3(nq), dim3(FU_THREADS), lds, st, a, n2);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

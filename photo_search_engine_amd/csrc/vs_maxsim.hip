// vs_maxsim.hip -- the kernels of the multi-vector search (include/vs.h "multi-vector search"; host:
// vs_maxsim_host.hip).
//
// A query is m sub-queries (1..FUSE_MAX_Q).  A group's score is F = ((M_0 + M_1) + ...) + M_{m-1} in fp64,
// M_j the best canonical score S_j over the group's members: a selection, so M_j is bit-equal to one
// member's score, and a sum of at most 8 terms in a fixed order.  Inside the kernels F is held as its key, F
// or -F for L2 (negation is exact), so "better" is always "greater" (fs_better).
//
// k_maxsim_walk: one workgroup per query.  Its candidates are the m exact top-L lists of row ids, turned
// into group codes, or the rank kernel's codes.  The codes are sorted (the bitonic network under a constant
// key), duplicates struck out and the N distinct ones packed to the front by a second sort.  Each wave then
// takes whole groups: it walks the group's member list in ascending id, passes over the rows the members'
// bitmap disallows, scores RR rows at a time against all m sub-queries (fuse_score_rows: every S_j is the
// canonical score bit for bit) and keeps per sub-query the best score and its id, replaced only by a
// strictly better one, so the lowest id that attains M_j stays.  Every group forms its F, the (F, code)
// pairs are sorted best first, and every group finds its rank by binary search and, below k, writes its
// outputs there.  The certificate is in DESIGN §7q.
// Every store is bounded: LDS by n2 >= nl L entries, the scratch rows by N <= nl L, the outputs by rank <
// k; a list entry at or past n_cov ends its list like an absent one, a code at or past ncodes is no
// candidate, member-list positions are cut to [0, n_cov].
//
// k_maxsim_scan: shaped like k_range_scan.  A workgroup takes a slice of the covered rows (or of the
// members' id list), queries go over gridDim.y.  Each wave-step scores RR rows against the m sub-queries
// once; after the butterfly every lane holds every sum, so lane j RR + i offers S_j of row i to
// table[q][j][code] with a 64-bit atomicMax of ms_key(S).  (A relaxed load in front of the atomic, to spare it
// once a better key is there, measured 1-3 % slower and is left in as a measurement variant only.)
//
// k_maxsim_rank: one workgroup per query decodes each code's m keys, forms F in the fixed order and keeps
// the k best under (F, code); the walk then recomputes everything for those codes, so both tiers end in
// the same kernel.  Plain vector stores and HIP atomics only.
#include "vs_fuse_score.h"
#include "vs_scan.h"

namespace vs {

constexpr int MS_THREADS = 512;  // k_maxsim_walk, k_maxsim_rank: one workgroup per query
constexpr int MS_NW = MS_THREADS / 64;
constexpr size_t MS_SCAN_QLDS = LDS_QUERY_BUDGET;  // the scan stages the sub-queries as fp64 in LDS up to this size
static_assert(FUSE_WALK_MAX <= 32 * MS_THREADS, "the duplicate mask keeps one bit per entry of a thread");
static_assert(FUSE_MAX_Q <= MS_NW, "the certificate rescoring gives every list's last entry a wave");

// The table's key: an order-preserving image of the fp64 score on 64 bits, inverted for L2 so that greater
// is better under either metric.  A non-negative S maps to its bits with the sign bit set, a negative one
// to the complement of its bits.  0 is the image of the bit pattern ~0 (inner product) or 0x7FFF...F (L2),
// both NaNs: no finite S maps to 0, which therefore means "no member".  Every accumulator of
// fuse_score_rows starts at +0.0 and x + (+0.0) is never -0.0, so no S is -0.0 and the order of the keys is
// the order of the scores.
template <int METRIC>
__device__ __forceinline__ unsigned long long ms_key(double S) {
    unsigned long long u = (unsigned long long)__double_as_longlong(S);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return METRIC == METRIC_IP ? u : ~u;
}
template <int METRIC>
__device__ __forceinline__ double ms_unkey(unsigned long long u) {
    if (METRIC != METRIC_IP) u = ~u;
    u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
    return __longlong_as_double((long long)u);
}

// the dense code of a row's group: its index among the distinct keys, or G + u for the u-th ungrouped row
__device__ __forceinline__ uint32_t ms_code(int32_t gid, int64_t G) {
    return gid >= 0 ? (uint32_t)gid : (uint32_t)(G + (int64_t)(~gid));
}

// qv [m][d] fp32 -> qs [m][8][ng] fp64
__device__ __forceinline__ void ms_stage_queries(double* qs, const float* qv, int m, int d, int ng, int tid, int nthreads) {
    for (int i = tid; i < m * d; i += nthreads) {
        const int j = i / d, e = i - j * d;
        qs[((size_t)j * 8 + (e & 7)) * ng + (e >> 3)] = (double)qv[i];
    }
}

// ---- the walk ------------------------------------------------------------------------------------
template <int DT, int METRIC, bool QLDS>
__global__ void __launch_bounds__(MS_THREADS) k_maxsim_walk(MaxsimWalkArgs a, int n2) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [key fp64 n2 | sub-queries fp64 m 8 ng | code n2]
    constexpr int RR = refine_rows<DT>();
    __shared__ int s_len[FUSE_MAX_Q];
    __shared__ double s_u[FUSE_MAX_Q];
    __shared__ int s_n, s_dup, s_nv;
    __shared__ unsigned long long s_rows;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ng = (a.d + 7) >> 3;
    const int m = a.m, nl = a.nl, L = (int)a.L, NE = nl * L;  // NE <= n2
    double* key = (double*)smem;
    double* qs = key + n2;
    uint32_t* eid = (uint32_t*)(qs + (QLDS ? (size_t)m * 8 * ng : 0));
    const int64_t* Cl = a.cand + q * (int64_t)NE;
    const float* qv = a.q + q * (int64_t)m * a.d;
    double* Mt = a.M_tmp + q * (int64_t)NE * m;
    uint32_t* It = a.I_tmp + q * (int64_t)NE * m;
    uint32_t* Ct = a.C_tmp + q * (int64_t)NE;
    int32_t* Zt = a.Z_tmp + q * (int64_t)NE;
    int64_t* Ko = a.keys + q * a.k;
    double* Fo = a.F + q * a.k;
    float* Do = a.D_sub + q * (int64_t)a.k * m;
    int64_t* Io = a.I_sub + q * (int64_t)a.k * m;
    int64_t* Zo = a.sizes + q * a.k;
    const int64_t G = a.g.G, ncodes = a.g.ncodes, n_cov = a.g.n_cov;
    if (tid < FUSE_MAX_Q) s_len[tid] = L;
    if (tid == 0) {
        s_n = 0;
        s_dup = 0;
        s_nv = 0;
        s_rows = 0ull;
    }
    if constexpr (QLDS) ms_stage_queries(qs, qv, m, a.d, ng, tid, MS_THREADS);
    __syncthreads();
    // a list ends at its first absent entry (a row at or past n_cov is no member: it ends it too)
    const int64_t cbound = a.codes ? ncodes : n_cov;
    for (int p = tid; p < NE; p += MS_THREADS) {
        const int64_t id = Cl[p];
        if (id < 0 || id >= cbound) atomicMin(&s_len[p / L], p % L);
    }
    __syncthreads();
    for (int p = tid; p < n2; p += MS_THREADS) {
        bool in = p < NE && p % L < s_len[p / L];
        uint32_t c = 0xFFFFFFFFu;
        if (in) {
            c = a.codes ? (uint32_t)Cl[p] : ms_code(a.g.gid[Cl[p]], G);
            in = (int64_t)c < ncodes;
        }
        key[p] = in ? 0.0 : -INFINITY;
        eid[p] = in ? c : 0xFFFFFFFFu;
    }
    __syncthreads();
    // the codes ascending (one key, so the order is the code's), the absent ones behind; then every repeat
    // of a code is struck out and a second sort packs the distinct ones to the front
    sort_best_first<METRIC_IP>(key, eid, n2);
    __syncthreads();
    {
        uint32_t dup = 0u;
        int cnt = 0;
        for (int p = tid, i = 0; p < n2; p += MS_THREADS, ++i) {
            const uint32_t c = eid[p];
            if (c == 0xFFFFFFFFu) continue;
            if (p > 0 && eid[p - 1] == c) dup |= 1u << i;
            else ++cnt;
        }
        __syncthreads();  // (every neighbour is read before any entry is struck out)
        for (int p = tid, i = 0; p < n2; p += MS_THREADS, ++i)
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
    const int N = s_n;  // distinct candidate groups, <= NE
    // the candidate groups' rows, from the offsets, before anything is scored
    {
        unsigned long long rows = 0ull;
        for (int p = tid; p < N; p += MS_THREADS) {
            const uint32_t c = eid[p];
            Ct[p] = c;
            const int64_t i0 = a.g.ml_off[c], i1 = a.g.ml_off[c + 1];
            if (i1 > i0) rows += (unsigned long long)(i1 - i0);
        }
        if (rows) atomicAdd(&s_rows, rows);
    }
    __syncthreads();
    const int64_t total = (int64_t)s_rows;
    if (tid == 0) a.walked[q] = total;
    if (!a.codes && !a.hold_all && total > a.walk_rows) {  // (block-uniform) over the cap: the scan answers it
        if (tid == 0) a.complete[q] = 2;
        return;
    }
    // every wave takes whole groups
    for (int p = wid; p < N; p += MS_NW) {
        const uint32_t c = eid[p];
        int64_t i = a.g.ml_off[c], i1 = a.g.ml_off[c + 1];
        i = i < 0 ? 0 : i;
        i1 = i1 > n_cov ? n_cov : i1;
        double bs[FUSE_MAX_Q];
        uint32_t bi[FUSE_MAX_Q];
#pragma unroll
        for (int j = 0; j < FUSE_MAX_Q; ++j) {
            bs[j] = 0.0;
            bi[j] = 0xFFFFFFFFu;
        }
        int cnt = 0;
        while (i < i1) {  // (wave-uniform: every lane reads the same list)
            int64_t rr[RR];
#pragma unroll
            for (int r = 0; r < RR; ++r) {
                rr[r] = -1;
                while (i < i1 && rr[r] < 0) {  // (no branch around the assignment: a select)
                    const int64_t row = (int64_t)a.g.ml_rows[i++];
                    unsigned long long word = ~0ull;
                    if (a.sel_bits) word = row < a.n_sel ? a.sel_bits[row >> 6] : 0ull;
                    const bool ok = row < n_cov && ((word >> (row & 63)) & 1ull) != 0ull;
                    rr[r] = ok ? row : -1;
                }
            }
            if (rr[0] < 0) break;
            double s[FUSE_MAX_Q][RR];
            fuse_score_rows<DT, METRIC, QLDS, RR>(a.corpus, rr, qs, qv, m, a.d, a.dpad, lane, s);
#pragma unroll
            for (int r = 0; r < RR; ++r) {
                if (rr[r] < 0) continue;
#pragma unroll
                for (int j = 0; j < FUSE_MAX_Q; ++j)
                    if (j < m) {
                        const bool better = cnt == 0 || (METRIC == METRIC_IP ? s[j][r] > bs[j] : s[j][r] < bs[j]);
                        if (better) {
                            bs[j] = s[j][r];
                            bi[j] = (uint32_t)rr[r];
                        }
                    }
                ++cnt;
            }
        }
        if (lane == 0) {
            Zt[p] = cnt;
#pragma unroll
            for (int j = 0; j < FUSE_MAX_Q; ++j)
                if (j < m) {
                    Mt[(size_t)p * m + j] = bs[j];
                    It[(size_t)p * m + j] = bi[j];
                }
        }
    }
    __syncthreads();
    // F in the fixed order, as its key
    auto fkey = [&](int p) {
        double f = Mt[(size_t)p * m];
        for (int j = 1; j < m; ++j) f = f + Mt[(size_t)p * m + j];
        return METRIC == METRIC_L2 ? -f : f;
    };
    {
        int cnt = 0;
        for (int p = tid; p < N; p += MS_THREADS) {
            const bool has = Zt[p] > 0;  // a group with no member under the selector does not exist
            key[p] = has ? fkey(p) : -INFINITY;
            cnt += has ? 1 : 0;
        }
        if (cnt) atomicAdd(&s_nv, cnt);
    }
    __syncthreads();
    if (N > 0) sort_valid_best_first<METRIC_IP>(key, eid, N, n2);
    __syncthreads();
    const int Nv = s_nv;
    const float worst = METRIC == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
    for (int p = tid; p < N; p += MS_THREADS) {
        if (Zt[p] <= 0) continue;
        const uint32_t c = Ct[p];
        const double f = fkey(p);
        const int r = fs_rank(key, eid, N, f, c);
        if (r < a.k) {
            Ko[r] = (int64_t)c < G ? a.g.gkey[c] : a.g.ukey[(int64_t)c - G];
            Fo[r] = METRIC == METRIC_L2 ? -f : f;
            Zo[r] = (int64_t)Zt[p];
            for (int j = 0; j < m; ++j) {
                Do[(size_t)r * m + j] = (float)Mt[(size_t)p * m + j];
                Io[(size_t)r * m + j] = (int64_t)It[(size_t)p * m + j];
            }
        }
    }
    for (int r = Nv + tid; r < a.k; r += MS_THREADS) {
        Ko[r] = -0x7FFFFFFFFFFFFFFFll - 1;
        Fo[r] = METRIC == METRIC_L2 ? (double)INFINITY : -(double)INFINITY;
        Zo[r] = 0;
        for (int j = 0; j < m; ++j) {
            Do[(size_t)r * m + j] = worst;
            Io[(size_t)r * m + j] = -1;
        }
    }
    // the certificate: a group no list touched has, for every j, M_j no better than list j's last entry
    // S_{j,L}; rounding and addition are monotone, so its F is no better than U, their sum in F's order
    bool open = !a.codes && !a.hold_all;  // (block-uniform) every list full: the bound decides
    if (open)
        for (int j = 0; j < nl; ++j) open = open && s_len[j] == L;
    if (open && Nv >= a.k && wid < nl) {  // (wave-uniform) wave j rescores list j's last entry
        int64_t rr[RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) rr[r] = -1;
        rr[0] = Cl[wid * L + L - 1];  // (a full list: below n_cov)
        double s[FUSE_MAX_Q][RR];
        fuse_score_rows<DT, METRIC, QLDS, RR>(a.corpus, rr, qs, qv, m, a.d, a.dpad, lane, s);
        double sj = 0.0;
#pragma unroll
        for (int j = 0; j < FUSE_MAX_Q; ++j)
            if (j == wid) sj = s[j][0];
        if (lane == 0) s_u[wid] = sj;
    }
    __syncthreads();
    if (tid == 0) {
        bool done = true;
        if (open) {
            done = false;
            if (Nv >= a.k) {
                double u = s_u[0];
                for (int j = 1; j < nl; ++j) u = u + s_u[j];
                done = key[a.k - 1] > (METRIC == METRIC_L2 ? -u : u);
            }
        }
        a.complete[q] = done ? 1 : 0;
    }
}

size_t maxsim_walk_lds(int64_t n_entries, int d, int m, bool* qlds) {
    const size_t base = pow2_at_least(n_entries, 64) * 12, qbytes = (size_t)m * query_lds_bytes(d);
    const bool fits = base + qbytes <= FUSE_DYN_CAP;
    if (qlds) *qlds = fits;
    return fits ? base + qbytes : base;
}

hipError_t launch_maxsim_walk(const MaxsimWalkArgs& a, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    const int64_t n = (int64_t)a.nl * a.L;
    if (a.k < 1 || a.k > FUSE_WALK_MAX || a.m < 1 || a.m > FUSE_MAX_Q || (a.nl != 1 && a.nl != a.m) || a.L < 1 ||
        n > FUSE_WALK_MAX || a.d < 1 || !a.corpus || !a.q || !a.cand || a.n_valid < 1 || a.n_valid > 0xFFFFFFFFll ||
        a.g.n_cov < 1 || a.g.n_cov > a.n_valid || a.g.ncodes < 1 || a.g.ncodes > a.g.n_cov || a.g.G < 0 ||
        a.g.G > a.g.ncodes || !a.g.gid || !a.g.ml_rows || !a.g.ml_off || !a.g.gkey || !a.g.ukey || !a.M_tmp || !a.I_tmp ||
        !a.C_tmp || !a.Z_tmp || !a.keys || !a.F || !a.D_sub || !a.I_sub || !a.sizes || !a.complete || !a.walked ||
        (a.metric != METRIC_IP && a.metric != METRIC_L2) || (a.codes && a.nl != 1) || (a.sel_bits && a.n_sel < 0))
        return hipErrorInvalidValue;
    bool qlds;
    const size_t lds = maxsim_walk_lds(n, a.d, a.m, &qlds);
    if (lds > FUSE_DYN_CAP) return hipErrorInvalidValue;
    const int n2 = (int)pow2_at_least(n, 64);
    const bool known = dispatch(a.dt, a.metric, qlds, [&](auto dt, auto metric, auto qlds_c) {
        launch_kernel(k_maxsim_walk<dt, metric, qlds_c>, (int)FUSE_DYN_CAP, dim3(nq), dim3(MS_THREADS), lds, st, a, n2);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

// ---- the scan ------------------------------------------------------------------------------------
template <int DT, int METRIC, bool QLDS, bool SEL>
__global__ void __launch_bounds__(FS_THREADS) k_maxsim_scan(MaxsimScanArgs a, const uint32_t* __restrict__ ids,
                                                            int64_t n_ids) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double* qs = (double*)smem;
    constexpr int RR = refine_rows<DT>();
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.x, G = gridDim.x;
    const int ng = (a.d + 7) >> 3;
    const int m = a.m;
    const int64_t n_cov = a.g.n_cov, ncodes = a.g.ncodes;
    const int64_t nseq = SEL ? n_ids : n_cov;
    const int64_t r0 = nseq * b / G, r1 = nseq * (b + 1) / G;
    for (int q = blockIdx.y; q < a.nq; q += gridDim.y) {
        __syncthreads();  // (the previous query's readers of qs are done)
        const float* qv = a.q + (int64_t)q * m * a.d;
        if constexpr (QLDS) ms_stage_queries(qs, qv, m, a.d, ng, tid, FS_THREADS);
        __syncthreads();
        unsigned long long* tq = a.table + (int64_t)q * m * ncodes;
        for (int64_t base = r0; base < r1; base += FS_NW * RR) {
            int64_t rr[RR];
#pragma unroll
            for (int i = 0; i < RR; ++i) {
                const int64_t r = base + wid + (int64_t)i * FS_NW;
                int64_t id = -1;
                if (r < r1) id = SEL ? (int64_t)ids[r] : r;
                rr[i] = id < n_cov ? id : -1;  // (the ids ascend: past n_cov every later one is, too)
            }
            if (rr[0] < 0) continue;  // (wave-uniform)
            double s[FUSE_MAX_Q][RR];
            fuse_score_rows<DT, METRIC, QLDS, RR>(a.corpus, rr, qs, qv, m, a.d, a.dpad, lane, s);
            // every lane holds every sum: lane j RR + i offers S_j of row i
            auto offer = [&](int j, int64_t row, double sc) {
                if (row < 0 || row >= n_cov) return;
                const int64_t code = (int64_t)ms_code(a.g.gid[row], a.g.G);
                if (code >= ncodes) return;
                const unsigned long long key = ms_key<METRIC>(sc);
                unsigned long long* p = tq + (int64_t)j * ncodes + code;
                // (measurement only: a relaxed load in front of the atomic; DESIGN §7q has the A/B it lost)
                if (!(a.variant & 2) || __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(p, key);
            };
            if (a.variant & 1) {  // (measurement only: lane 0 offers every pair)
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < FUSE_MAX_Q; ++j)
#pragma unroll
                        for (int i = 0; i < RR; ++i)
                            if (j < m) offer(j, rr[i], s[j][i]);
                }
            } else {
                double mine = 0.0;
                int64_t row = -1;
                int jj = 0;
#pragma unroll
                for (int j = 0; j < FUSE_MAX_Q; ++j)
#pragma unroll
                    for (int i = 0; i < RR; ++i)
                        if (j < m && lane == j * RR + i) {
                            mine = s[j][i];
                            row = rr[i];
                            jj = j;
                        }
                offer(jj, row, mine);
            }
        }
    }
}

hipError_t launch_maxsim_scan(const MaxsimScanArgs& a, const uint32_t* ids, int64_t n_ids, int G, int qy, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (qy < 1 || qy > a.nq || qy > 65535 || G < 1 || a.m < 1 || a.m > FUSE_MAX_Q || a.d < 1 || !a.corpus || !a.q ||
        !a.table || !a.g.gid || a.g.n_cov < 1 || a.g.n_cov > 0xFFFFFFFFll || a.g.ncodes < 1 || a.g.G < 0 ||
        (ids && n_ids <= 0) || (a.metric != METRIC_IP && a.metric != METRIC_L2))
        return hipErrorInvalidValue;
    const size_t qbytes = (size_t)a.m * query_lds_bytes(a.d);
    const bool qlds = qbytes <= MS_SCAN_QLDS;
    const dim3 grid(G, qy), block(FS_THREADS);
    // (the sub-queries in global memory: no dynamic LDS, and the default limit serves)
    const bool known = dispatch(a.dt, a.metric, qlds, ids != nullptr, [&](auto dt, auto metric, auto qlds_c, auto sel) {
        launch_kernel(k_maxsim_scan<dt, metric, qlds_c, sel>, qlds_c ? LDS_DYN_MAX : 0, grid, block, qlds_c ? qbytes : 0, st,
                      a, ids, n_ids);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

// ---- the rank ------------------------------------------------------------------------------------
// LDS: (key, code)[n2], n2 a power of two >= k + MS_THREADS.  [0, k) is the running list, best first;
// candidates better than its k-th entry are appended behind it (at most MS_THREADS per step, and a step
// starts only with that much room), and a full buffer is sorted: the best k are the list again.
template <int METRIC>
__global__ void __launch_bounds__(MS_THREADS) k_maxsim_rank(const unsigned long long* __restrict__ table, int m,
                                                            int64_t ncodes, int k, int n2, int64_t* __restrict__ cand) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_fill;
    double* key = (double*)smem;
    uint32_t* eid = (uint32_t*)(key + n2);
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const unsigned long long* tq = table + q * (int64_t)m * ncodes;
    for (int p = tid; p < n2; p += MS_THREADS) {
        key[p] = -INFINITY;
        eid[p] = 0xFFFFFFFFu;
    }
    if (tid == 0) s_fill = 0;
    __syncthreads();
    const int room = n2 - k;  // >= MS_THREADS
    int fill = 0;
    for (int64_t c0 = 0; c0 < ncodes; c0 += MS_THREADS) {
        if (fill + MS_THREADS > room) {  // (block-uniform)
            sort_best_first<METRIC_IP>(key, eid, n2);
            __syncthreads();
            for (int p = k + tid; p < n2; p += MS_THREADS) {
                key[p] = -INFINITY;
                eid[p] = 0xFFFFFFFFu;
            }
            if (tid == 0) s_fill = 0;
            __syncthreads();
            fill = 0;
        }
        const double tf = key[k - 1];
        const uint32_t tc = eid[k - 1];
        const int64_t c = c0 + tid;
        if (c < ncodes) {
            const unsigned long long u0 = tq[c];
            if (u0 != 0ull) {  // (a group with a member has every one of its m keys)
                double f = ms_unkey<METRIC>(u0);
                for (int j = 1; j < m; ++j) f = f + ms_unkey<METRIC>(tq[(int64_t)j * ncodes + c]);
                const double kf = METRIC == METRIC_L2 ? -f : f;
                if (fs_better(kf, (uint32_t)c, tf, tc)) {
                    const int pos = atomicAdd(&s_fill, 1);  // < fill + MS_THREADS <= room
                    key[k + pos] = kf;
                    eid[k + pos] = (uint32_t)c;
                }
            }
        }
        __syncthreads();
        fill = s_fill;
        __syncthreads();  // (every thread has read the count before the next step adds to it)
    }
    sort_best_first<METRIC_IP>(key, eid, n2);
    __syncthreads();
    for (int r = tid; r < k; r += MS_THREADS) cand[q * k + r] = eid[r] != 0xFFFFFFFFu ? (int64_t)eid[r] : -1;
}

hipError_t launch_maxsim_rank(const unsigned long long* table, int nq, int m, int64_t ncodes, int metric, int k,
                              int64_t* cand, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (!table || !cand || m < 1 || m > FUSE_MAX_Q || ncodes < 1 || ncodes > 0xFFFFFFFEll || k < 1 || k > K_MAX ||
        (metric != METRIC_IP && metric != METRIC_L2))
        return hipErrorInvalidValue;
    const int n2 = (int)pow2_at_least(k + MS_THREADS, 1024);
    const size_t lds = (size_t)n2 * 12;
    const bool known = with_metric(metric, [&](auto metric_c) {
        launch_kernel(k_maxsim_rank<metric_c>, 0, dim3(nq), dim3(MS_THREADS), lds, st, table, m, ncodes, k, n2, cand);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

// vs_scan.h -- the streaming exact scan shared by k_full_scan (vs_fullscan.hip: every row of the
// shard), k_sel_scan (vs_selscan.hip: the rows of a selector's ascending id list), k_adjust_scan
// (vs_adjust.hip: either sequence, ranked by a per-row affine function of the score), k_fuse_scan
// (vs_fuse.hip: either sequence, each row scored against several sub-queries at once and ranked by the
// best or the worst of those scores) and k_after_scan (vs_after.hip: either sequence, the rows at or
// before a query's cursor passed over and counted): the bounded running top-k under the total order (score, then id),
// its batch sort / rank merge, and the last workgroup's merge of the per-workgroup lists (st_agent /
// ld_agent hand-off).
//
// Workgroup b scans positions [n b / G, n (b + 1) / G) of its row sequence -- row ids themselves
// (SEL = false) or entries of the id list (SEL = true).  Either sequence ascends in id, so once a
// workgroup's list is full a row tied with its k-th best never enters it: the memory stays O(k)
// however many rows tie, and the merged answer is the k lowest ids among equal scores.
#pragma once
#include <type_traits>

#include "vs_device.h"
#include "vs_dispatch.h"

namespace vs {

constexpr int FS_NW = FS_THREADS / 64;  // (FS_THREADS, FS_B: vs_internal.h)
static_assert(FS_B == FS_THREADS, "the batch sort keeps one element per thread");

__device__ __forceinline__ bool fs_better(double sa, uint32_t ia, double sb, uint32_t ib) {
    return sa != sb ? sa > sb : ia < ib;
}
// entries of the best-first list (sc, id)[0, n) better than (s, i)
__device__ __forceinline__ int fs_rank(const double* sc, const uint32_t* id, int n, double s, uint32_t i) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (fs_better(sc[mid], id[mid], s, i)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct FsLists {
    double* lsc[2];
    uint32_t* lid[2];
    double* bsc;
    uint32_t* bid;
};

// merge the best-first batch (bsc, bid)[0, nb) into list `cur` (nl entries), keeping the best k in
// list cur ^ 1; every thread updates cur / nl alike
__device__ __forceinline__ void fs_merge(const FsLists& L, int& cur, int& nl, int nb, int k) {
    const int tid = threadIdx.x;
    const double* asc = L.lsc[cur];
    const uint32_t* aid = L.lid[cur];
    double* osc = L.lsc[cur ^ 1];
    uint32_t* oid = L.lid[cur ^ 1];
    for (int i = tid; i < nb; i += FS_THREADS) {
        const double s = L.bsc[i];
        const uint32_t id = L.bid[i];
        const int p = i + fs_rank(asc, aid, nl, s, id);
        if (p < k) {
            osc[p] = s;
            oid[p] = id;
        }
    }
    for (int j = tid; j < nl; j += FS_THREADS) {
        const double s = asc[j];
        const uint32_t id = aid[j];
        const int p = j + fs_rank(L.bsc, L.bid, nb, s, id);
        if (p < k) {
            osc[p] = s;
            oid[p] = id;
        }
    }
    __syncthreads();
    cur ^= 1;
    nl = min(k, nl + nb);
}

// sort the batch's nb entries (by rank; the bitonic network over the next power of two, worst-padded,
// past one entry per thread) and merge them in
__device__ __forceinline__ void fs_sort_merge(const FsLists& L, int& cur, int& nl, int nb, int k) {
    int n2 = 1;
    while (n2 < nb) n2 <<= 1;
    for (int j = nb + (int)threadIdx.x; j < n2; j += FS_THREADS) {
        L.bsc[j] = -INFINITY;
        L.bid[j] = 0xFFFFFFFFu;
    }
    __syncthreads();
    sort_valid_best_first<METRIC_IP>(L.bsc, L.bid, nb, n2);
    fs_merge(L, cur, nl, nb, k);
}

// rows per wave in flight: twice the refine's (one workgroup per CU here, so the registers are there)
template <int DT>
constexpr int fs_rows() { return DT == DT_F32 ? 4 : 8; }

// dynamic LDS of one scan workgroup: two k-lists and the batch (KL = k's power of two, >= 64), and
// the query -- a fused scan's m sub-queries -- as fp64 when it fits beside them (qlds)
inline size_t fs_lds_bytes(int k, int d, int m, int* KL_out, bool* qlds_out) {
    const int KL = (int)pow2_at_least(k, 64);
    const size_t base = (size_t)KL * 24 + (size_t)FS_B * 12;
    const size_t qbytes = (size_t)m * query_lds_bytes(d);
    const bool qlds = base + qbytes <= LDS_QUERY_BUDGET;
    *KL_out = KL;
    *qlds_out = qlds;
    return qlds ? base + qbytes : base;
}

// (the hand-off of the workgroups' lists to the last one: st_agent / ld_agent, vs_device.h)

// The scan of one launch: SEL = false scores rows [0, a.n_valid); SEL = true the sel_m rows
// sel_ids[0, sel_m) (ascending, each < a.n_valid), and the grid's y dimension deals the queries
// (slice y takes queries y, y + gridDim.y, ...: a short list fills few workgroups per query, and a
// query's lists, counter and outputs are its own).
// XF: what a row's canonical score becomes before the running top-k.  FsPlain ranks by the score itself
// and compiles to nothing; an active transform (vs_adjust.hip) may pass a row over, or put another key
// in the score's place -- the key is what the lists hold and what D / S64 report.
// A fused transform (`static constexpr bool fused = true`, vs_fuse.hip) scores a row itself, against
// xf.m sub-queries in one pass: a.q holds m vectors per query, load_queries stages them as fp64 (QLDS: m
// times the query's LDS), and score_rows returns per row the one score the lists rank by.  It scores the
// refine's rows per wave, not the scan's (m accumulators per row).
// A per-query transform (`static constexpr bool per_query = true`, vs_after.hip) gets the query's index
// in its key hook and may count the rows it passes over: key(q, id, s, passed) adds to the lane's
// `passed`, and count(q, n) takes the workgroup's sum once per query.
// Every hook below is an `if constexpr`: a transform that is neither compiles to the code it had without
// them.
struct FsPlain {
    static constexpr bool active = false;
};
template <class XF, class = void>
struct fs_per_query : std::false_type {};
template <class XF>
struct fs_per_query<XF, std::void_t<decltype(XF::per_query)>> : std::bool_constant<XF::per_query> {};
template <class XF, class = void>
struct fs_fused : std::false_type {};
template <class XF>
struct fs_fused<XF, std::void_t<decltype(XF::fused)>> : std::bool_constant<XF::fused> {};
template <int DT, int METRIC, bool QLDS, bool SEL, class XF = FsPlain>
__device__ __forceinline__ void fs_scan_body(const FullScanArgs& a, int KL, const uint32_t* __restrict__ sel_ids,
                                             int64_t sel_m, const XF& xf = XF()) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (a.gate && *a.gate == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.x, G = gridDim.x;
    const int ng = (a.d + 7) >> 3;
    FsLists L;
    L.lsc[0] = (double*)smem;
    L.lsc[1] = L.lsc[0] + KL;
    L.bsc = L.lsc[1] + KL;
    double* qs = L.bsc + FS_B;
    constexpr bool FUSED = fs_fused<XF>::value;
    if constexpr (FUSED) L.lid[0] = (uint32_t*)(qs + (QLDS ? (size_t)ng * 8 * xf.m : 0));
    else L.lid[0] = (uint32_t*)(qs + (QLDS ? (size_t)ng * 8 : 0));
    L.lid[1] = L.lid[0] + KL;
    L.bid = L.lid[1] + KL;
    __shared__ int go_s, nb_s, last_s;
    __shared__ int red_s[FS_NW];
    constexpr bool PERQ = fs_per_query<XF>::value;
    __shared__ unsigned passed_s;  // (PERQ: the rows this workgroup's transform passed over and counted)
    constexpr int RR = FUSED ? refine_rows<DT>() : fs_rows<DT>();
    const int k = a.k;
    const int64_t nseq = SEL ? sel_m : a.n_valid;
    const int64_t r0 = nseq * b / G, r1 = nseq * (b + 1) / G;
    constexpr bool QY = SEL || FUSED;  // (a fused scan deals its queries over the grid's y dimension either way)
    const int qfirst = QY ? (int)blockIdx.y : 0, qstep = QY ? (int)gridDim.y : 1;
    for (int q = qfirst; q < a.nq; q += qstep) {
        __syncthreads();  // (the previous query's readers of qs / the lists are done)
        if (tid == 0) {
            go_s = (a.all_queries || a.cert[q] == 0) ? 1 : 0;
            nb_s = 0;
            if constexpr (PERQ) passed_s = 0u;
        }
        __syncthreads();
        if (!go_s) continue;
        const float* qv = a.q + (int64_t)q * a.d;
        if constexpr (FUSED) qv = a.q + (int64_t)q * a.d * xf.m;
        if constexpr (QLDS) {
            if constexpr (FUSED) xf.load_queries(qs, qv, a.d, ng, tid);
            else
                for (int i = tid; i < a.d; i += FS_THREADS) qs[(i & 7) * ng + (i >> 3)] = (double)qv[i];
        }
        __syncthreads();
        int cur = 0, nl = 0;
        [[maybe_unused]] unsigned passed = 0u;
        for (int64_t base = r0; base < r1; base += FS_NW * RR) {
            int64_t rr[RR];
#pragma unroll
            for (int i = 0; i < RR; ++i) {
                const int64_t r = base + wid + (int64_t)i * FS_NW;
                if constexpr (SEL) rr[i] = r < r1 ? (int64_t)sel_ids[r] : -1;
                else rr[i] = r < r1 ? r : -1;
            }
            if (rr[0] >= 0) {  // (wave-uniform)
                double s4[RR];
                if constexpr (FUSED) xf.template score_rows<DT, METRIC, QLDS, RR>(a, rr, qs, qv, lane, s4);
                else exact_score_rows<DT, METRIC, QLDS, RR>(a.corpus, rr, qs, qv, a.d, a.dpad, lane, s4);
                if (lane == 0) {
                    const bool full = nl >= k;
                    const double ts = full ? L.lsc[cur][k - 1] : 0.0;
                    const uint32_t ti = full ? L.lid[cur][k - 1] : 0u;
#pragma unroll
                    for (int i = 0; i < RR; ++i) {
                        if (rr[i] < 0) continue;
                        double s = METRIC == METRIC_L2 ? -s4[i] : s4[i];
                        const uint32_t id = (uint32_t)rr[i];
                        if constexpr (PERQ) {
                            if (!xf.template key<METRIC>(q, id, s, passed)) continue;
                        } else if constexpr (XF::active) {
                            if (!xf.template key<METRIC>(id, s4[i], s)) continue;
                        }
                        if (!full || fs_better(s, id, ts, ti)) {
                            const int slot = atomicAdd(&nb_s, 1);
                            L.bsc[slot] = s;
                            L.bid[slot] = id;
                        }
                    }
                }
            }
            __syncthreads();
            const int nb = nb_s;
            if (nb > FS_B - FS_NW * RR || base + FS_NW * RR >= r1) {
                if (nb > 0) fs_sort_merge(L, cur, nl, nb, k);
                if (tid == 0) nb_s = 0;
                __syncthreads();
            }
        }
        if constexpr (PERQ)
            if (lane == 0 && passed) atomicAdd(&passed_s, passed);
        // this workgroup's list -> scratch; the last workgroup of the query merges all of them
        double* gs = a.gsc + ((size_t)q * G + b) * k;
        uint32_t* gi = a.gid + ((size_t)q * G + b) * k;
        for (int j = tid; j < k; j += FS_THREADS) {
            st_agent(gs + j, j < nl ? L.lsc[cur][j] : -INFINITY);
            st_agent(gi + j, j < nl ? L.lid[cur][j] : 0xFFFFFFFFu);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (every storing wave, before the add)
        __syncthreads();
        if constexpr (PERQ)
            if (tid == 0 && passed_s) xf.count(q, passed_s);
        if (tid == 0)
            last_s = __hip_atomic_fetch_add(a.gdone + q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                             (unsigned)(G - 1) ? 1 : 0;
        __syncthreads();
        if (!last_s) continue;
        // The other lists as one flat array [G][k].  First a floor: the k-th best of the G lists'
        // heads (k distinct rows at least that good, so no entry below it can be in the top-k).  Then
        // FS_B entries at a time (the next chunk's loads in flight): entries at least as good as the
        // floor that beat the running k-th best are appended to the batch; a batch that would
        // overflow, and the last one, are sorted and merged (few entries pass the floor).
        {
            const double* vs_ = a.gsc + (size_t)q * G * k;
            const uint32_t* vi = a.gid + (size_t)q * G * k;
            const int total = G * k;
            // every load of the first FS_PF chunks (and the heads) issued before any is used
            constexpr int FS_PF = 8;
            auto fetch = [&](int j, double& s, uint32_t& id) {
                s = -INFINITY;
                id = 0xFFFFFFFFu;
                if (j < total && j / k != b) {
                    s = ld_agent(vs_ + j);
                    id = ld_agent(vi + j);
                }
            };
            double ps[FS_PF];
            uint32_t pi[FS_PF];
#pragma unroll
            for (int c = 0; c < FS_PF; ++c) fetch(c * FS_B + tid, ps[c], pi[c]);
            int h2 = 1;
            while (h2 < G) h2 <<= 1;
            for (int g = tid; g < h2; g += FS_THREADS) {
                double s = -INFINITY;
                uint32_t id = 0xFFFFFFFFu;
                if (g < G) {
                    if (g == b) {
                        if (nl > 0) {
                            s = L.lsc[cur][0];
                            id = L.lid[cur][0];
                        }
                    } else {
                        s = ld_agent(vs_ + (size_t)g * k);
                        id = ld_agent(vi + (size_t)g * k);
                    }
                }
                L.bsc[g] = s;
                L.bid[g] = id;
            }
            __syncthreads();
            sort_valid_best_first<METRIC_IP>(L.bsc, L.bid, G, h2);
            const bool has_floor = G >= k && L.bid[k - 1] != 0xFFFFFFFFu;
            const double fs = has_floor ? L.bsc[k - 1] : -INFINITY;
            const uint32_t fi = has_floor ? L.bid[k - 1] : 0xFFFFFFFFu;
            __syncthreads();  // (every thread has the floor before the batch is reused)
            int nb = 0;  // entries waiting in the batch (block-uniform)
            for (int c0 = 0, ci = 0; c0 < total; c0 += FS_B, ++ci) {
                const int slot = ci % FS_PF;
                double s = 0.0;
                uint32_t id = 0u;
#pragma unroll
                for (int c = 0; c < FS_PF; ++c)
                    if (c == slot) {
                        s = ps[c];
                        id = pi[c];
                    }
                if (slot == FS_PF - 1)  // this group of chunks is in registers: fetch the next group
#pragma unroll
                    for (int c = 0; c < FS_PF; ++c) fetch(c0 + (c + 1) * FS_B + tid, ps[c], pi[c]);
                bool ok = id != 0xFFFFFFFFu;
                if (ok && has_floor) ok = !fs_better(fs, fi, s, id);  // not below the floor
                if (ok && nl >= k) ok = fs_better(s, id, L.lsc[cur][k - 1], L.lid[cur][k - 1]);
                const u64 m = __ballot(ok);
                if (lane == 0) red_s[wid] = __popcll(m);
                __syncthreads();
                int wb = 0, cnt = 0;
                for (int i = 0; i < FS_NW; ++i) {
                    if (i < wid) wb += red_s[i];
                    cnt += red_s[i];
                }
                if (nb + cnt > FS_B) {  // (block-uniform) make room
                    fs_sort_merge(L, cur, nl, nb, k);
                    nb = 0;
                }
                if (ok) {
                    const int pos = nb + wb + lane_prefix(m);
                    L.bsc[pos] = s;
                    L.bid[pos] = id;
                }
                nb += cnt;
                __syncthreads();
            }
            if (nb > 0) fs_sort_merge(L, cur, nl, nb, k);
        }
        const size_t ost = a.ostride > 1 ? (size_t)a.ostride : 1;
        for (int j = tid; j < k; j += FS_THREADS) {
            const size_t o = (size_t)q * k + j;
            if (j < nl) {
                const double v = METRIC == METRIC_L2 ? -L.lsc[cur][j] : L.lsc[cur][j];
                if (a.D) a.D[o] = (float)v;
                a.I[o * ost] = (int64_t)L.lid[cur][j] + a.id_offset;
                if (a.S64) a.S64[o * ost] = v;
            } else {
                if (a.D) a.D[o] = METRIC == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
                a.I[o * ost] = -1;
                if (a.S64) a.S64[o * ost] = METRIC == METRIC_L2 ? 1.7976931348623157e308 : -1.7976931348623157e308;
            }
        }
        if (tid == 0) {
            a.cert[q] = 1;
            st_agent(a.gdone + q, 0u);  // ready for the next launch
            if (a.count) atomicAdd(a.count, 1u);
        }
    }
}

// ---- the launcher ------------------------------------------------------------------------------------
// what every scan over fs_scan_body asks of its arguments
inline bool fs_args_ok(const FullScanArgs& a) {
    return a.nq > 0 && a.k > 0 && a.k <= KP_MAX && a.G > 0 && a.G <= FS_B && a.n_valid > 0 && a.cert && a.I && a.gsc &&
           a.gid && a.gdone && a.q && a.corpus && (a.metric == METRIC_IP || a.metric == METRIC_L2);
}

// One launch of a scan kernel: the shared checks, the LDS rule (m: the sub-queries staged per query), the grid
// a.G x ny and the dtype x metric x QLDS x SEL dispatch.  pick(dt, metric, qlds, sel) names the kernel; its
// arguments are (a, KL, extra...).  What a scan adds stays in its own launch_*_scan: its own checks, ny and sel.
template <class PICK, class... EXTRA>
hipError_t fs_launch_scan(const FullScanArgs& a, int m, bool sel, int ny, hipStream_t st, PICK&& pick,
                          const EXTRA&... extra) {
    if (!fs_args_ok(a)) return hipErrorInvalidValue;
    int KL;
    bool qlds;
    const size_t lds = fs_lds_bytes(a.k, a.d, m, &KL, &qlds);
    const dim3 grid(a.G, ny), block(FS_THREADS);
    const bool known = dispatch(a.dt, a.metric, qlds, sel, [&](auto dt, auto metric, auto qlds_c, auto sel_c) {
        launch_kernel(pick(dt, metric, qlds_c, sel_c), LDS_DYN_MAX, grid, block, lds, st, a, KL, extra...);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

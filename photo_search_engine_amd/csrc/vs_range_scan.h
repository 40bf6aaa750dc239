// vs_range_scan.h -- the range scan and the range refine kernels, shared by the range search
// (vs_range.hip: passing rows appended to a pair buffer), the facet counts (vs_facet.hip: passing rows
// counted into a per-group histogram), the duplicate groups (vs_components.hip: passing rows united with
// the query's own row in a union-find) and the score selectors (vs_scoresel.hip: passing rows set a bit of
// a bitmap) and the density clusters (vs_dbscan.hip: passing rows counted into both ends' degrees, then
// united or offered as a border row's core neighbour).  One K loop, one exact_score_rows call and one predicate; what
// happens to a row that passes is the business of the SINK, a template parameter built from its own
// kernel argument (SINK::Args) and the workgroup's dynamic LDS:
//   begin(a, q)      every thread, per query: the query's state (the pair sink's region)
//   open(tid)        every thread, per query, between the two barriers that fence the staged query
//   put<..>(..)      lane 0 of a wave: its R scored rows
//   close(q, tid)    every thread, after the query's last row (the next query's first barrier follows)
// The pair sink's open / close are empty and take no barrier: a plain range search compiles to the code
// it always ran.  The launchers of both kernels, for any sink, are at the end of the file.
#pragma once
#include <type_traits>

#include "vs_scan.h"

namespace vs {

constexpr size_t RS_QLDS_MAX = 48 * 1024;  // the fp64 query is staged in LDS up to this size

__device__ __forceinline__ bool rs_pass(double S, float r, int metric) {
    const float D = (float)S;
    return metric == METRIC_IP ? D > r : D < r;
}

// queries taken from stored rows: may row `id` be returned to the query gathered from row `self`?
// (mode VS_SELF_KEEP for every plain range search: always)
__device__ __forceinline__ bool rs_self_ok(int64_t id, int64_t self, int mode) {
    return mode == VS_SELF_DROP ? id != self : mode == VS_SELF_ABOVE ? id > self : true;
}

// lane 0 of a wave: append the passing rows among its R scored rows to query q's region
// (SELF: the queries are stored rows; without it the self fields are not read and a plain range
// search compiles to the code it always ran)
template <int METRIC, int R, bool SELF>
__device__ __forceinline__ void rs_append(const RangeArgs& a, int q, float rq, int64_t off, int64_t cap,
                                          int64_t self, const int64_t (&rr)[R], const double (&s)[R]) {
    unsigned pass = 0u;
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (rr[i] >= 0 && (!SELF || rs_self_ok(rr[i], self, a.self_mode)) && rs_pass(s[i], rq, METRIC)) pass |= 1u << i;
    if (!pass) return;
    unsigned long long pos = atomicAdd(a.cnt + q, (unsigned long long)__popc(pass));
#pragma unroll
    for (int i = 0; i < R; ++i)
        if ((pass >> i) & 1u) {
            if ((int64_t)pos < cap) {
                a.psc[off + (int64_t)pos] = s[i];
                a.pid[off + (int64_t)pos] = (uint32_t)rr[i];
            }
            ++pos;
        }
}

// the range search's sink: (S, id) pairs into the query's region of the pair buffer
struct RsPairSink {
    struct Args {};
    __device__ __forceinline__ RsPairSink(const Args&, uint8_t*) {}
    struct Q {
        int64_t off, cap;
    };
    __device__ __forceinline__ Q begin(const RangeArgs& a, int q) const { return {a.off[q], a.cap[q]}; }
    __device__ __forceinline__ void open(int) const {}
    template <int METRIC, int R, bool SELF>
    __device__ __forceinline__ void put(const RangeArgs& a, int q, float rq, const Q& st, int64_t self,
                                        const int64_t (&rr)[R], const double (&s)[R]) const {
        rs_append<METRIC, R, SELF>(a, q, rq, st.off, st.cap, self, rr, s);
    }
    __device__ __forceinline__ void close(int, int) const {}
};

// the facet counts' sink: hist[q][bin] += 1 per passing member, bin = the row's group code, or G for an
// ungrouped row (gid null: the one bin 0).  Rows at or past n_cov are no members (a selector made after
// the groups allows them; the screen lists them).  LDS = false: one device atomic per distinct bin among
// the wave-step's R rows.  LDS = true: the workgroup's own uint32 bins (a workgroup scores fewer than
// 2^31 rows per query), zeroed in open(), flushed in close() -- the non-zero ones -- with one device
// atomic each.  Every index is below `bins`, the row length the host sized hist by.
template <bool LDS>
struct RsCountSink {
    struct Args {
        FacetArgs f;
        int bins_off;  // LDS form: the bins' byte offset in dynamic LDS (behind the staged query)
    };
    FacetArgs f;
    unsigned* lbins;  // LDS form: [bins]
    __device__ __forceinline__ RsCountSink(const Args& sa, uint8_t* smem)
        : f(sa.f), lbins((unsigned*)(smem + sa.bins_off)) {}
    struct Q {};
    __device__ __forceinline__ Q begin(const RangeArgs&, int) const { return {}; }
    __device__ __forceinline__ void open(int tid) const {
        if constexpr (LDS)
            for (int b = tid; b < f.bins; b += FS_THREADS) lbins[b] = 0u;
    }
    template <int METRIC, int R, bool SELF>
    __device__ __forceinline__ void put(const RangeArgs&, int q, float rq, const Q&, int64_t, const int64_t (&rr)[R],
                                        const double (&s)[R]) const {
        static_assert(!SELF, "facet counts take no queries from stored rows");
        unsigned pass = 0u;
        int bin[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            bin[i] = 0;
            if (rr[i] >= 0 && rr[i] < f.n_cov && rs_pass(s[i], rq, METRIC)) {
                pass |= 1u << i;
                if (f.gid) {
                    const int c = f.gid[rr[i]];
                    bin[i] = c >= 0 && c < f.bins - 1 ? c : f.bins - 1;
                }
            }
        }
        if (!pass) return;
        if constexpr (LDS) {
#pragma unroll
            for (int i = 0; i < R; ++i)
                if ((pass >> i) & 1u) atomicAdd(lbins + bin[i], 1u);
        } else {
            unsigned long long* row = f.hist + (int64_t)q * f.bins;
#pragma unroll
            for (int i = 0; i < R; ++i)
                if ((pass >> i) & 1u) {
                    unsigned n = 1u;
#pragma unroll
                    for (int j = i + 1; j < R; ++j)
                        if (((pass >> j) & 1u) && bin[j] == bin[i]) {
                            ++n;
                            pass &= ~(1u << j);
                        }
                    atomicAdd(row + bin[i], (unsigned long long)n);
                }
        }
    }
    __device__ __forceinline__ void close(int q, int tid) const {
        if constexpr (LDS) {
            __syncthreads();  // (every wave's adds of this query are in)
            unsigned long long* row = f.hist + (int64_t)q * f.bins;
            for (int b = tid; b < f.bins; b += FS_THREADS) {
                const unsigned v = lbins[b];
                if (v) atomicAdd(row + b, (unsigned long long)v);
            }
        }
    }
};

// ---- duplicate groups: lock-free union-find over parent[0, n) (vs_components.hip) -----
// Every access to `parent` while unions run is a relaxed agent-scope atomic: the array is its own and only
// payload, so no ordering against other memory is needed, only that each word is read and written whole
// and past this CU's L1.
__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree.  Follows parent until parent[r] == r; with HALVE, points the nodes of the path at
// their grandparents on the way -- a value this thread has read as an ancestor of that node, hence smaller
// than the node and an ancestor of it for ever (trees only ever merge at their roots).  A store goes to a
// non-root only (its parent was read as another node, and a non-root never becomes a root again), so it
// never meets a CAS that hooks a root.
template <bool HALVE>
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
    uint32_t p = cc_load(parent + x);
    while (p != x) {
        const uint32_t g = cc_load(parent + p);
        if (HALVE && g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// Join the trees of x and y.
// Invariant: parent[v] <= v for every v, with equality exactly at roots.  k_cc_init sets parent[v] = v;
// path halving stores an ancestor, which is smaller; a hook stores the smaller of two distinct roots under
// the larger.  A path therefore descends strictly and ends, and the root of a tree is its minimum id:
// once all edges are in, find(v) is the smallest id of v's component whatever order the unions took --
// the labels do not depend on the schedule, the tier or the grid.
// Hook: roots hi > lo are joined by atomicCAS(parent + hi, hi, lo), which succeeds only while hi still is
// a root, so a root is hooked once and no union is lost.  lo needs no check: were it hooked meanwhile (or
// read from a stale line), hi hangs under a former root of the same tree that x and y now share.  On
// failure the CAS returns hi's new parent, an ancestor smaller than hi: the search goes on from there, so
// every failed round strictly lowers the pair and the loop ends (at the latest with both at the tree's
// minimum, where the roots are equal and nothing is left to do).  Uniting a joined pair again changes
// nothing: unions are idempotent.
__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t x, uint32_t y) {
    uint32_t a = cc_find<true>(parent, x), b = cc_find<true>(parent, y);
    while (a != b) {
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = cc_find<true>(parent, old);
        b = cc_find<true>(parent, lo);
    }
}

// the duplicate groups' sink (queries are stored rows under VS_SELF_ABOVE): a passing row is an edge
// (self, id) -- counted into the block's cnt[q] with one atomic per wave-step, and united with the query's
// own row.  The test is the pair sink's; ids index parent[0, n_valid) only (the scan's rows and a
// selector's ids are below n_valid, the refine drops keys at or past it, the self ids are member ids; put()
// bounds both again).
struct RsUnionSink {
    struct Args {
        uint32_t* parent;  // [n_valid]
    };
    uint32_t* parent;
    __device__ __forceinline__ RsUnionSink(const Args& sa, uint8_t*) : parent(sa.parent) {}
    struct Q {};
    __device__ __forceinline__ Q begin(const RangeArgs&, int) const { return {}; }
    __device__ __forceinline__ void open(int) const {}
    template <int METRIC, int R, bool SELF>
    __device__ __forceinline__ void put(const RangeArgs& a, int q, float rq, const Q&, int64_t self,
                                        const int64_t (&rr)[R], const double (&s)[R]) const {
        static_assert(SELF, "duplicate groups take their queries from stored rows");
        if (self < 0 || self >= a.n_valid) return;
        unsigned pass = 0u;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (rr[i] >= 0 && rr[i] < a.n_valid && rs_self_ok(rr[i], self, a.self_mode) && rs_pass(s[i], rq, METRIC))
                pass |= 1u << i;
        if (!pass) return;
        atomicAdd(a.cnt + q, (unsigned long long)__popc(pass));
#pragma unroll
        for (int i = 0; i < R; ++i)
            if ((pass >> i) & 1u) cc_unite(parent, (uint32_t)self, (uint32_t)rr[i]);
    }
    __device__ __forceinline__ void close(int, int) const {}
};

// ---- density clusters (vs_dbscan.hip) --------------------------------------------------
// Both sinks take their queries from stored rows under VS_SELF_ABOVE and apply the union sink's test; ids
// index deg / core / best / parent [0, n_valid) only, and put() bounds both ends again.

// pass 1, the neighbour counts: an edge (self, id) is one neighbour more for either end.  The wave-step's
// passing rows go to the block's cnt[q] with one atomic (the query's "edges above", which pass 2 reads to
// skip the queries that meet none), to deg[self] with one more, and each passing row's deg[id] gets 1.
// An add is not idempotent: the host gives every query to exactly one tier (range_tiers, vs_range_tiers.h).
struct RsDegreeSink {
    struct Args {
        uint32_t* deg;  // [n_valid], zeroed by the host
    };
    uint32_t* deg;
    __device__ __forceinline__ RsDegreeSink(const Args& sa, uint8_t*) : deg(sa.deg) {}
    struct Q {};
    __device__ __forceinline__ Q begin(const RangeArgs&, int) const { return {}; }
    __device__ __forceinline__ void open(int) const {}
    template <int METRIC, int R, bool SELF>
    __device__ __forceinline__ void put(const RangeArgs& a, int q, float rq, const Q&, int64_t self,
                                        const int64_t (&rr)[R], const double (&s)[R]) const {
        static_assert(SELF, "neighbour counts take their queries from stored rows");
        if (self < 0 || self >= a.n_valid) return;
        unsigned pass = 0u;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (rr[i] >= 0 && rr[i] < a.n_valid && rs_self_ok(rr[i], self, a.self_mode) && rs_pass(s[i], rq, METRIC))
                pass |= 1u << i;
        if (!pass) return;
        const unsigned c = (unsigned)__popc(pass);
        atomicAdd(a.cnt + q, (unsigned long long)c);
        atomicAdd(deg + self, c);
#pragma unroll
        for (int i = 0; i < R; ++i)
            if ((pass >> i) & 1u) atomicAdd(deg + rr[i], 1u);
    }
    __device__ __forceinline__ void close(int, int) const {}
};

// a border row's choice among its core neighbours as one 64-bit maximum: an order-preserving image of D
// (inverted for L2, so that greater is better under either metric) above the complement of the core row's id
// (so that of equal D the lower id wins).  -0.0f is folded into +0.0f first: the order is float equality's.
// A passing D is no NaN, so no key is 0: 0 in best[] means "no core neighbour".
template <int METRIC>
__device__ __forceinline__ unsigned long long db_key(double S, uint32_t core_id) {
    float D = (float)S;
    if (D == 0.0f) D = 0.0f;
    uint32_t u = __float_as_uint(D);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (METRIC != METRIC_IP) u = ~u;
    return ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)~core_id;
}
__device__ __forceinline__ uint32_t db_key_id(unsigned long long key) { return ~(uint32_t)key; }

// pass 2, the clusters: an edge with both ends core joins their trees (cc_unite: a tree's root is its
// smallest id, here its smallest core id); an edge with one end core offers that core row to the other end
// (atomicMax on best[border]); an edge between two non-core rows does nothing.  Unions and maxima are
// idempotent: a query answered twice changes nothing.  a.cnt is not touched: it holds pass 1's counts.
struct RsDbscanSink {
    struct Args {
        uint32_t* parent;          // [n_valid], parent[i] = i before the pass
        const uint8_t* core;       // [n_valid], 1 for a core row (k_db_core)
        unsigned long long* best;  // [n_valid], zeroed by the host
    };
    uint32_t* parent;
    const uint8_t* core;
    unsigned long long* best;
    __device__ __forceinline__ RsDbscanSink(const Args& sa, uint8_t*) : parent(sa.parent), core(sa.core), best(sa.best) {}
    struct Q {};
    __device__ __forceinline__ Q begin(const RangeArgs&, int) const { return {}; }
    __device__ __forceinline__ void open(int) const {}
    template <int METRIC, int R, bool SELF>
    __device__ __forceinline__ void put(const RangeArgs& a, int, float rq, const Q&, int64_t self,
                                        const int64_t (&rr)[R], const double (&s)[R]) const {
        static_assert(SELF, "density clusters take their queries from stored rows");
        if (self < 0 || self >= a.n_valid) return;
        unsigned pass = 0u;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (rr[i] >= 0 && rr[i] < a.n_valid && rs_self_ok(rr[i], self, a.self_mode) && rs_pass(s[i], rq, METRIC))
                pass |= 1u << i;
        if (!pass) return;
        const bool self_core = core[self] != 0;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if ((pass >> i) & 1u) {
                const bool id_core = core[rr[i]] != 0;
                if (self_core && id_core) cc_unite(parent, (uint32_t)self, (uint32_t)rr[i]);
                else if (self_core) atomicMax(best + rr[i], db_key<METRIC>(s[i], (uint32_t)self));
                else if (id_core) atomicMax(best + self, db_key<METRIC>(s[i], (uint32_t)rr[i]));
            }
    }
    __device__ __forceinline__ void close(int, int) const {}
};

// the score selectors' sink (vs_scoresel.hip): a passing row sets its bit in the query's bitmap,
// bits + q * stride_words -- stride 0 (ANY): the block's queries share one bitmap; stride = the bitmap's
// words (ALL): one bitmap per query of the block.  The rows of a wave-step are FS_NW apart, so several
// usually fall into one 64-bit word: their bits are merged, and per distinct word of a shared bitmap one
// relaxed agent-scope load decides whether an atomicOr is still needed (with many queries most are not).
// Bits only ever get set, so a stale load costs an atomic and never a bit.  Ids index
// bits[0, ceil(n_valid / 64)) only: put() bounds them again.
struct RsBitSink {
    struct Args {
        unsigned long long* bits;
        int64_t stride_words;
    };
    unsigned long long* bits;
    int64_t stride;
    __device__ __forceinline__ RsBitSink(const Args& sa, uint8_t*) : bits(sa.bits), stride(sa.stride_words) {}
    struct Q {};
    __device__ __forceinline__ Q begin(const RangeArgs&, int) const { return {}; }
    __device__ __forceinline__ void open(int) const {}
    template <int METRIC, int R, bool SELF>
    __device__ __forceinline__ void put(const RangeArgs& a, int q, float rq, const Q&, int64_t, const int64_t (&rr)[R],
                                        const double (&s)[R]) const {
        static_assert(!SELF, "score selectors keep the query's own row: no self id is read");
        unsigned pass = 0u;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (rr[i] >= 0 && rr[i] < a.n_valid && rs_pass(s[i], rq, METRIC)) pass |= 1u << i;
        if (!pass) return;
        unsigned long long* row = bits + (int64_t)q * stride;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if ((pass >> i) & 1u) {
                const int64_t w = rr[i] >> 6;
                unsigned long long mask = 1ull << (rr[i] & 63);
#pragma unroll
                for (int j = i + 1; j < R; ++j)
                    if (((pass >> j) & 1u) && (rr[j] >> 6) == w) {
                        mask |= 1ull << (rr[j] & 63);
                        pass &= ~(1u << j);
                    }
                // (a bitmap of the query's own: each of its bits is written once per tier, the load would find
                // nothing and only put a round trip in front of the atomic -- DESIGN §7o has the A/B)
                if (stride != 0 ||
                    (~__hip_atomic_load(row + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask) != 0ull)
                    atomicOr(row + w, mask);
            }
    }
    __device__ __forceinline__ void close(int, int) const {}
};

template <bool QLDS>
__device__ __forceinline__ void rs_stage_query(double* qs, const float* qv, int d, int ng) {
    if constexpr (QLDS)
        for (int i = threadIdx.x; i < d; i += FS_THREADS) qs[(i & 7) * ng + (i >> 3)] = (double)qv[i];
}

// ---- SCAN tier ------------------------------------------------------------------------------------
template <int DT, int METRIC, bool QLDS, bool SEL, bool SELF, class SINK = RsPairSink>
__global__ void __launch_bounds__(FS_THREADS) k_range_scan(RangeArgs a, const uint32_t* __restrict__ ids, int64_t m,
                                                           typename SINK::Args sa) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double* qs = (double*)smem;
    const SINK sink(sa, smem);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.x, G = gridDim.x;
    const int ng = (a.d + 7) >> 3;
    constexpr int RR = fs_rows<DT>();
    // (a self-join under VS_SELF_ABOVE: rows below row0 pass for no query of the block)
    const int64_t lo = SEL || !SELF ? 0 : a.row0;
    const int64_t nseq = SEL ? m : a.n_valid - lo;
    const int64_t r0 = lo + nseq * b / G, r1 = lo + nseq * (b + 1) / G;
    for (int q = blockIdx.y; q < a.nq; q += gridDim.y) {
        if (a.go && a.go[q] == 0) continue;  // (block-uniform)
        __syncthreads();                     // (the previous query's readers of qs are done)
        const float* qv = a.q + (int64_t)q * a.d;
        rs_stage_query<QLDS>(qs, qv, a.d, ng);
        sink.open(tid);
        __syncthreads();
        const float rq = a.radius[q];
        const typename SINK::Q sq = sink.begin(a, q);
        const int64_t self = SELF ? a.self[q] : -1;
        for (int64_t base = r0; base < r1; base += FS_NW * RR) {
            int64_t rr[RR];
#pragma unroll
            for (int i = 0; i < RR; ++i) {
                const int64_t r = base + wid + (int64_t)i * FS_NW;
                if constexpr (SEL) rr[i] = r < r1 ? (int64_t)ids[r] : -1;
                else rr[i] = r < r1 ? r : -1;
            }
            if (rr[0] < 0) continue;  // (wave-uniform)
            double s[RR];
            exact_score_rows<DT, METRIC, QLDS, RR>(a.corpus, rr, qs, qv, a.d, a.dpad, lane, s);
            if (lane == 0) sink.template put<METRIC, RR, SELF>(a, q, rq, sq, self, rr, s);
        }
        sink.close(q, tid);
    }
}

// ---- SCREEN tier: exact refine of the survivors ------------------------------------------------------
template <int DT, int METRIC, bool QLDS, bool SELF, class SINK = RsPairSink>
__global__ void __launch_bounds__(FS_THREADS) k_range_refine(RangeArgs a, const u64* __restrict__ glist,
                                                             const int* __restrict__ gcnt, int lcap,
                                                             typename SINK::Args sa) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double* qs = (double*)smem;
    const SINK sink(sa, smem);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int q = blockIdx.x;
    const int ng = (a.d + 7) >> 3;
    constexpr int RR = fs_rows<DT>();
    if (a.go && a.go[q] == 0) return;
    const int n = min(max(gcnt[q], 0), lcap);
    const float* qv = a.q + (int64_t)q * a.d;
    rs_stage_query<QLDS>(qs, qv, a.d, ng);
    __syncthreads();
    const u64* keys = glist + (size_t)q * lcap;
    const float rq = a.radius[q];
    const typename SINK::Q sq = sink.begin(a, q);
    const int64_t self = SELF ? a.self[q] : -1;
    for (int j0 = (int)blockIdx.y * FS_NW * RR; j0 < n; j0 += (int)gridDim.y * FS_NW * RR) {
        int64_t rr[RR];
        int first = -1;
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int j = j0 + wid + i * FS_NW;
            rr[i] = -1;
            if (j < n) {
                const u64 key = keys[j];
                const int64_t id = (int64_t)key_id(key);
                if (key != 0ull && id < a.n_valid) rr[i] = id;  // (never an address outside the shard)
            }
            if (first < 0 && rr[i] >= 0) first = i;
        }
        if (first < 0) continue;  // (wave-uniform)
        if (first > 0) {          // exact_score_rows reads row[0] whatever else is absent
#pragma unroll
            for (int i = 1; i < RR; ++i)
                if (i == first) {
                    rr[0] = rr[i];
                    rr[i] = -1;
                }
        }
        double s[RR];
        exact_score_rows<DT, METRIC, QLDS, RR>(a.corpus, rr, qs, qv, a.d, a.dpad, lane, s);
        if (lane == 0) sink.template put<METRIC, RR, SELF>(a, q, rq, sq, self, rr, s);
    }
}

// ---- launchers -------------------------------------------------------------------------------------
// One scan launcher and one refine launcher for every sink: the argument checks that no sink changes, the
// staged query's LDS rule and the dtype x metric x QLDS (x SEL) dispatch.  What a sink adds stays in its own
// .hip file, in the launch_*_scan / launch_*_refine wrapper of vs_internal.h: its SELF, the check of its own
// arguments, and (the count sink's LDS form alone) sink_lds, the bytes of dynamic LDS it takes behind the
// query, with lds_attr, the dynamic LDS limit its kernels are raised to (0: the default limit serves).

// the staged query's bytes of dynamic LDS; 0: the query is too long and stays in global memory (QLDS false)
inline size_t rs_query_lds(int d) {
    const size_t qbytes = query_lds_bytes(d);
    return qbytes <= RS_QLDS_MAX ? qbytes : 0;
}

inline bool rs_args_ok(const RangeArgs& a) {
    return a.corpus && a.q && a.radius && a.nq > 0 && a.d > 0 && a.n_valid > 0 &&
           (a.metric == METRIC_IP || a.metric == METRIC_L2) && a.row0 >= 0 && a.row0 < a.n_valid;
}

template <class SINK, bool SELF>
hipError_t rs_launch_scan(const RangeArgs& a, const typename SINK::Args& sa, size_t sink_lds, int lds_attr, int G, int qy,
                          const uint32_t* ids, int64_t m, hipStream_t st) {
    if (!rs_args_ok(a) || G < 1 || qy < 1 || qy > a.nq || qy > 65535 || m < 0 || (ids && m == 0) || (!ids && m != 0) ||
        (ids && a.row0 != 0))
        return hipErrorInvalidValue;
    const size_t qbytes = rs_query_lds(a.d), lds = qbytes + sink_lds;
    const dim3 grid(G, qy), block(FS_THREADS);
    const bool known = dispatch(a.dt, a.metric, qbytes != 0, ids != nullptr, [&](auto dt, auto metric, auto qlds,
                                auto sel) {
        launch_kernel(k_range_scan<dt, metric, qlds, sel, SELF, SINK>, lds_attr, grid, block, lds, st, a, ids, m, sa);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

template <class SINK, bool SELF>
hipError_t rs_launch_refine(const RangeArgs& a, const typename SINK::Args& sa, const u64* glist, const int* gcnt,
                            int lcap, int ny, hipStream_t st) {
    if (!rs_args_ok(a) || !glist || !gcnt || lcap <= 0 || ny < 1 || ny > 65535) return hipErrorInvalidValue;
    const size_t lds = rs_query_lds(a.d);
    const dim3 grid(a.nq, ny), block(FS_THREADS);
    const bool known = dispatch<false>(a.dt, a.metric, lds != 0, [&](auto dt, auto metric, auto qlds) {  // (no fp32 screen)
        launch_kernel(k_range_refine<dt, metric, qlds, SELF, SINK>, 0, grid, block, lds, st, a, glist, gcnt, lcap, sa);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

// vs_index.h -- the flat index object and its per-call contexts, shared by the host units of libvs
// (vs_store.hip, vs_search.hip, vs_sel_host.hip, vs_range_host.hip, vs_rows_host.hip, vs_probe.hip,
// vs_api.hip, vs_remove.hip, vs_kmeans.hip, vs_diverse_host.hip, vs_group_host.hip, vs_adjust_host.hip,
// vs_fuse_host.hip, vs_after_host.hip, vs_facet_host.hip, vs_components_host.hip, vs_scoresel_host.hip, vs_dbscan_host.hip; the
// five before the last four share the list-deepening driver of vs_walk.h; vs_range_host.hip and the last four
// share the tier driver of vs_range_tiers.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vs.h"
#include "vs_internal.h"

namespace vs {

// pinned staging per context for the host-buffer search (queries in, results out)
constexpr size_t kPinnedStageCap = 8u << 20;

// per-call execution context: stream + workspace (pooled; one per concurrent search)
struct Ctx {
    hipStream_t stream = nullptr;
    // recorded behind the last lease's work on its caller's stream: the next lease (possibly on
    // another stream) waits on it before touching the workspace, so a device-API search that
    // returned with kernels still queued is never overwritten by the next caller's pack
    hipEvent_t idle = nullptr;
    bool pending = false;
    DevBuf qdev, qtile, qinfo, qpad, cand, part, merge_a, merge_b, outD, outI, outS, cert, thr0, seedmax, gcnt, gT;
    DevBuf qfac, qeps, drop;  // int8 screen: per-query code scale and norm, refine margin, drop bounds
    DevBuf fails;             // the current query block's certificate-failure counts: [0] first pass (the
                              // fallback round's gate), [1] fallback round (the full scan's gate)
    DevBuf fsc, fdone;        // full scan: per-workgroup lists of the block's queries, done counters
    DevBuf selD, selI, selS;  // filtered search, overfetch tier: the unfiltered exact lists [nq][k']
    DevBuf selaux;            // ... its certificates, allowed counts and proven flags ([3][nq] ints)
    DevBuf rng_p[2];          // range search: the pair buffers (first pass; reruns of overflowed queries)
    DevBuf rng_aux;           // ... the block's radii, go flags, counters, regions and segments
    DevBuf rng_D, rng_I, rng_S;  // ... the block's emitted results
    DevBuf row_ids;           // queries taken from stored rows: the call's ids, uploaded once
    DevBuf row_out;           // ... a chunk's lists without the rows themselves ([I int64 | D fp32], k_rows_take)
    DevBuf dv_out;            // diversified search: the walk's radii and outputs
    DevBuf gr_out;            // grouped search: the walk's outputs
    DevBuf rsc, rdone;        // split refine: per-query scores + ids of the kept rows, done counters
    DevBuf pa;       // two-phase (sharded) search: the refine's phase-1 state between the launches
    DevBuf rows[2];  // read_rows_host: unpacked fp32 chunks
    DevBuf tilectr;  // GEMV screen: tile work-queue counter
    DevBuf seedacc;  // MFMA seed pass: raw accumulators of each workgroup's seed tile
    DevBuf outAll;   // vs_search: I (int64), D (fp32), certificates in one block: ONE D2H copy
    // the device fallback round's query tile, packed ahead by the block's first pass: 0 none (the
    // round packs it), 1 the native first pass's own tile (qtile), 2 the int8 pass's native copy
    // (qtile_n); the round's list counters are gcnt2 / drop2, zeroed by the same pack
    DevBuf qtile_n, gcnt2, drop2;
    int prepacked = 0;
    PinnedPair pin;  // read_rows_host: pinned landing chunks
    HostBuf hq;      // vs_search: the query batch, staged for the H2D copy
    HostBuf hout;    // vs_search: I (int64), D (fp32) and certificates land here; search_exact_device: certificates
    unsigned* unres = nullptr;  // this call's full-scan counter (device), instead of the index's
    ~Ctx() {  // (the buffers free themselves; the owner has the device current and idle)
        if (idle) hipEventDestroy(idle);
        if (stream) hipStreamDestroy(stream);
    }
};

// A walk job on the index (diversified, grouped, adjusted, fused, paged search): the list lengths set by the caller
// (0 = the defaults) and what the last call reported, stats[] and its HIP-event ms times[].
struct WalkState {
    std::atomic<int> first{0}, limit{0};
    std::mutex mu;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double times[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    struct Depth { int64_t first, limit; };  // the first list's length and the longest one's
    Depth resolve(int64_t default_first, int kmax) const {
        const int set_first = first.load(), set_limit = limit.load();
        const int64_t lim = set_limit > 0 ? set_limit : kmax;
        return {std::min<int64_t>(set_first > 0 ? set_first : default_first, lim), lim};
    }
    void set(int new_first, int new_limit, int kmax, const char* what) {
        const std::string rule = " depth: 1 <= first <= limit <= " + std::to_string(kmax) + " (0 = default)";
        if (new_first < 0 || new_limit < 0 || new_first > kmax || new_limit > kmax ||
            (new_first > 0 && new_limit > 0 && new_first > new_limit))
            throw VsError(VS_ERR_ARG, what + rule);
        first.store(new_first);
        limit.store(new_limit);
    }
    void note(const int64_t* s, int ns, const double* t, int nt) {
        std::lock_guard<std::mutex> g(mu);
        std::copy(s, s + ns, stats);
        std::copy(t, t + nt, times);
    }
};

// the first min(n, cap) numbers a call left behind (the *_last_stats / *_last_times exports; what:
// "stats" or "times")
template <typename T>
void copy_last(std::mutex& mu, const T* src, int n, T* out, int cap, const char* what) {
    if (!out || cap < 0) throw VsError(VS_ERR_ARG, std::string("bad ") + what + " buffer");
    std::lock_guard<std::mutex> g(mu);
    std::copy(src, src + std::min(cap, n), out);
}

}  // namespace vs

constexpr int64_t kDefaultScanLimit = 192ll << 20;  // (the MALL holds such a corpus between calls)

struct vs_index {
    int d = 0, dpad = 0, metric = 0, dtype = 0, device = 0, es = 4;
    int num_cu = 256;
    int64_t ntotal = 0, cap_rows = 0;
    uint8_t* data = nullptr;
    float* sqn = nullptr;
    unsigned* d_maxsq = nullptr;
    unsigned* d_uncert = nullptr;
    unsigned* d_unres = nullptr;  // queries answered by the exact full scan (no bounded screen certified them)
    float maxsq = 0.0f;
    // int8 screen copy (VS_SCREEN_I8): codes in row tiles of 64-element chunks + per-row scale and
    // error norm; d_maxsq[2..3] = max ||x_hat||, max error norm (fp32 bits, certificate margins);
    // d_maxsq[8] = min ||x_hat|| (the query credit); every word: vs_internal.h IX_WORDS
    int screen = VS_SCREEN_NATIVE;
    int dpad8 = 0;
    int64_t cap8 = 0;
    uint8_t* data8 = nullptr;
    uint32_t* rsb = nullptr;  // per row: bf16 scale | bf16 error norm (rounded up) << 16
    float i8_bmax = 0.0f;     // host copy of the largest row error norm (int8 GEMV depth)
    // group residuals (inner product, direct int8 screen): bf16 means of I8_GROUP_ROWS-row groups
    // [gcap][dpad8] the codes are taken against (zero for groups without a mean worth it);
    // d_maxsq[5] = max ||mu_g|| (fp32 bits), d_maxsq[6] = groups that have a mean
    uint16_t* gmean = nullptr;
    int64_t gcap = 0;
    bool i8_res = false;  // some group has a mean: the int8 screen adds <mu_g, q> to its keys
    hipStream_t own = nullptr;  // ingest stream
    vs::DevBuf stage[2];           // add_rows_host: fp32 chunks on the device ...
    vs::PinnedPair pin;         // ... and their pinned host sources
    std::shared_mutex rw;       // shared: search; exclusive: add/reset
    std::mutex pool_mtx;
    std::vector<vs::Ctx*> pool_free;
    std::vector<vs::Ctx*> pool_all;
    // timing (bench): events around the screen kernel
    std::atomic<bool> timing{false};
    std::mutex tmtx;
    std::vector<std::pair<vs::DevEvent, vs::DevEvent>> tev;
    // corpora of at most this many stored bytes answer calls of 1-2 queries with the exact full scan
    // alone (vs_set_scan_limit; 0 = never)
    std::atomic<int64_t> scan_limit{kDefaultScanLimit};
    // id selectors (vs_search_sel): a selector records the reset generation it was made in; the tier
    // forced by vs_set_sel_mode; the last filtered search's {m, tier, k', re-answered} (vs_sel_last_stats)
    std::atomic<uint64_t> reset_gen{0};
    std::atomic<int> sel_mode{VS_SEL_AUTO};
    std::mutex sel_mu;
    int64_t sel_stats[4] = {0, 0, 0, 0};
    // range search: the tier forced by vs_set_range_mode; the last range search's {total, tier,
    // re-answered by the scan, host-sorted segments} (vs_range_last_stats)
    std::atomic<int> range_mode{VS_RANGE_AUTO};
    std::mutex range_mu;
    int64_t range_stats[4] = {0, 0, 0, 0};
    // diversified search (vs_set_diverse_depth): the last call's {queries, complete after the first
    // list, after a deeper list, answered from the full ranking, longest list walked}
    // (vs_diverse_last_stats) and its ms {search, walk} per tier (vs_diverse_last_times)
    vs::WalkState dv;
    // grouped search (vs_set_group_depth): the last call's {queries, complete after the first list,
    // after a deeper list, finished by restricted rounds, restricted rounds run, longest list walked}
    // (vs_group_last_stats) and its ms {search, walk} per tier, restrict, compact (vs_group_last_times)
    vs::WalkState gr;
    // adjusted search (vs_set_adjust_depth, vs_set_adjust_mode): the last call's {queries, complete after
    // the first list, after a deeper list, answered by the scan, longest list walked, tier taken, adjusted
    // rows} (vs_adjust_last_stats) and its ms {search, walk} per list tier, direct scan, full scan
    // (vs_adjust_last_times)
    vs::WalkState aj;
    std::atomic<int> adjust_mode{VS_ADJUST_AUTO};
    // fused search (vs_set_fuse_depth, vs_set_fuse_mode): the last call's {fused queries, complete after the
    // first list, after a deeper list, answered by the scan, longest list walked, tier taken}
    // (vs_fuse_last_stats) and its ms {search, walk} per list tier, scan, the scan's walk (vs_fuse_last_times)
    vs::WalkState fu;
    std::atomic<int> fuse_mode{VS_FUSE_AUTO};
    // multi-vector search (vs_set_maxsim_depth, vs_set_maxsim_mode): the last call's {queries, complete after
    // the first list, after a deeper list, answered by the scan, longest list walked, tier taken, candidate
    // rows walked} (vs_maxsim_last_stats) and its ms {search, walk} per list tier, scan, rank, the scan's walk
    // (vs_maxsim_last_times); the row cap of one walk (0 = default)
    vs::WalkState mx;
    std::atomic<int> maxsim_mode{VS_MAXSIM_AUTO};
    std::atomic<int64_t> maxsim_walk_rows{0};
    // paged search (vs_set_after_depth, vs_set_after_mode): the last call's {queries, complete after the
    // first list, after a deeper list, answered by the scan, longest list walked, tier taken}
    // (vs_after_last_stats) and its ms {search, cut} per list tier, cursor scoring, scan (vs_after_last_times)
    vs::WalkState af;
    std::atomic<int> after_mode{VS_AFTER_AUTO};
    // facet counts (vs_set_facet_hist): the last call's {sum of totals, tier taken, queries re-answered by the
    // scan, histogram form the scan took, query blocks} (vs_facet_last_stats) and its ms {screen + refine,
    // scan, table readback} (vs_facet_last_times)
    std::atomic<int> facet_hist{VS_FACET_HIST_AUTO};
    std::mutex facet_mu;
    int64_t facet_stats[5] = {0, 0, 0, 0, 0};
    double facet_times[3] = {0, 0, 0};
    // score selectors: the last vs_sel_from_range / _rows call's {allowed rows, members, tier taken, queries
    // re-answered by the scan, query blocks} (vs_scoresel_last_stats) and its ms {screen + refine, scan,
    // finish} (vs_scoresel_last_times)
    std::mutex ss_mu;
    int64_t ss_stats[5] = {0, 0, 0, 0, 0};
    double ss_times[3] = {0, 0, 0};
    // duplicate groups: the last call's {members, edges, components, tier taken, queries re-answered by the
    // scan, query blocks} (vs_components_last_stats) and its ms {gather + screen + refine, scan, flatten +
    // readback} (vs_components_last_times)
    std::mutex cc_mu;
    int64_t cc_stats[6] = {0, 0, 0, 0, 0, 0};
    double cc_times[3] = {0, 0, 0};
    // density clusters: the last vs_range_degrees / vs_range_dbscan call's {members, edges, clusters, core,
    // border, noise, tier taken, queries pass 1 gave to the scan after a screen overflow, query blocks, the
    // same of pass 2, query blocks pass 2 ran, pass-2 queries skipped} (vs_dbscan_last_stats) and its ms {pass 1
    // gather + screen + refine, pass 1 scan, pass 2 the same two, labels + readback} (vs_dbscan_last_times)
    std::mutex db_mu;
    int64_t db_stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double db_times[5] = {0, 0, 0, 0, 0};
    int last_kernel_kind = 0;  // 1 = mfma, 2 = gemv, 3 = int8 mfma, 4 = int8 gemv, 5 = exact full scan
    // Screen health (first passes of MFMA batches): the certificate-failure count of a batch is read
    // back without a host wait (pinned word + event, observed by a later search).  A failed query
    // costs its block a full fallback round, so the index adapts to its corpus:
    //  * an int8 batch with failures doubles the int8 union (the rows listed above the seed), up
    //    to 2^kI8ScaleMax; one failing at that depth routes the next kI8RouteBatches searches to
    //    the native screen (score distributions denser than the int8 error window, e.g. tight
    //    clusters); kSeedRelax clean int8 batches halve the depth again;
    //  * a native batch with a failed query doubles the optimistic seed's depth (rows listed ahead
    //    of the refine), up to 2^kSeedScaleMax; kSeedRelax clean batches halve it again.
    std::mutex h_mu;
    unsigned* h_fails = nullptr;  // pinned
    hipEvent_t h_ev = nullptr;
    int h_pending = 0;          // 0 none, 1 int8 batch, 2 native batch in flight
    int h_nq = 0;               // queries of that batch
    int h_clean = 0;            // consecutive clean readbacks (past kHealthCleanRun: every kHealthStride-th batch read)
    unsigned h_seq = 0;         // batches noted since
    int i8_route = 0;           // searches still routed to the native screen
    int seed_log2 = 0, seed_clean = 0;
    int i8_log2 = 0, i8_clean = 0;  // int8 union depth: 2^i8_log2 times the target (dense corpora)
    int i8_route_log2 = 0;          // consecutive routings (each twice as long as the last)
};

// ---- id selectors: exact filtered search (include/vs.h "id selectors"; kernels: vs_selscan.hip) ----
struct vs_sel {
    vs_index* ix = nullptr;
    uint64_t gen = 0;          // the index's reset generation at creation
    int device = 0;
    int64_t n_sel = 0, m = 0;  // rows covered, rows allowed
    uint64_t* bits = nullptr;  // device: ceil(n_sel / 64) words (zero past the uploaded bytes)
    uint32_t* ids = nullptr;   // device: the m allowed ids, ascending
};

// ---- group keys: exact grouped search (include/vs.h "grouped search"; kernels: vs_group.hip) ----
struct vs_groups {
    vs_index* ix = nullptr;
    uint64_t gen = 0;  // the index's reset generation at creation
    int device = 0;
    int64_t n_cov = 0, G = 0, U = 0;  // rows covered, distinct non-negative keys, ungrouped rows
    vs::DevBuf gid;    // int32 [n_cov] group codes (vs_internal.h)
    vs::DevBuf gkey;   // int64 [G] keys, ascending
    vs::DevBuf gsize;  // int32 [G] rows per group
    vs::DevBuf ukey;   // int64 [U] keys of the ungrouped rows, in row order
    // the member lists, made under ml_mu by the first multi-vector call with the object (vs_maxsim_host.hip);
    // a group's code is its index in gkey, or G + u for the u-th ungrouped row
    mutable std::mutex ml_mu;
    mutable bool ml_built = false;
    mutable vs::DevBuf ml_rows;  // uint32 [n_cov] the covered rows by (code, id)
    mutable vs::DevBuf ml_off;   // int64 [G + U + 1] where each code's rows begin
};

// ---- score adjustment: exact adjusted search (include/vs.h "adjusted search"; kernels: vs_adjust.hip) ----
struct vs_adjust {
    vs_index* ix = nullptr;
    uint64_t gen = 0;  // the index's reset generation at creation
    int device = 0;
    int64_t n_cov = 0, m_adj = 0;  // rows covered, rows that are not plain
    vs::DevBuf scale, bias;        // fp32 [n_cov]
    vs::DevBuf ids;                // uint32 [m_adj] the adjusted rows, ascending
    vs::DevBuf ext;                // fp32 [4] smin, smax, bmin, bmax over the covered rows (host copy below)
    float smin = 1.0f, smax = 1.0f, bmin = 0.0f, bmax = 0.0f;
};

namespace vs {

// the context pool of an index (vs_store.hip): a context is owned by the pool from its creation on
// (freed by vs_destroy)
Ctx* acquire_ctx(vs_index* ix);
void release_ctx(vs_index* ix, Ctx* c);

// vs_store.hip, shared with vs_remove.hip (the caller holds the exclusive lock, the device current).
// quantize_rows: the int8 screen copy of rows [r0, r0 + n) once they are in place, stream-ordered
// on st; with group residuals the groups they fall in get their means recomputed over every row
// below r0 + n and are requantised from their first row.  refresh_maxsq: the host copies of the
// device maxima (synchronises the ingest stream).
void quantize_rows(vs_index* ix, int64_t r0, int64_t n, hipStream_t st);
void refresh_maxsq(vs_index* ix);
void reset_i8_stats(vs_index* ix, hipStream_t st);  // maxima 0, min ||s c|| +inf: before a re-quantisation of every row

// A leased context works on `st` (null = the context's own stream): the lease first orders `st`
// behind the previous lease's work, and on release records the context's idle event on `st`.
struct CtxLease {
    vs_index* ix;
    Ctx* c;
    hipStream_t st;
    CtxLease(vs_index* i, hipStream_t s, bool own_stream) : ix(i), c(acquire_ctx(i)) {
        st = own_stream ? c->stream : s;
        if (c->pending) {
            hipError_t e = hipStreamWaitEvent(st, c->idle, 0);
            if (e != hipSuccess) {
                release_ctx(ix, c);
                HIP_CHECK(e);
            }
        }
    }
    ~CtxLease() {
        c->pending = hipEventRecord(c->idle, st) == hipSuccess;
        release_ctx(ix, c);
    }
};

inline void check_index(const vs_index* ix) {
    if (!ix) throw VsError(VS_ERR_ARG, "null index");
}

// one radius per query, none of them NaN
inline void check_radii(const float* radius, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (std::isnan(radius[i])) throw VsError(VS_ERR_ARG, "radius is NaN (query " + std::to_string(i) + ")");
}

// Points a leased Ctx's full-scan counter at the caller's device word for one call, and
// clears it on every exit (exceptions included), before the Ctx returns to the pool: a later
// lease must never count into a buffer it does not own.
struct UnresScope {
    Ctx* c;
    UnresScope(Ctx* c_, unsigned* unres) : c(c_) { c->unres = unres; }
    ~UnresScope() { c->unres = nullptr; }
    UnresScope(const UnresScope&) = delete;
    UnresScope& operator=(const UnresScope&) = delete;
};

// ---- vs_search.hip ----
// where a search writes: device [nq][k] arrays (D, S64 and cert may be null)
struct SearchOut {
    float* D = nullptr;
    int64_t* I = nullptr;
    double* S64 = nullptr;
    int* cert = nullptr;
    int64_t id_offset = 0;
    int ostride = 1;  // I / S64 element stride (RefineArgs::ostride)
    // the same view from query q0 on (null members stay null)
    SearchOut at(int64_t q0, int k) const {
        SearchOut o = *this;
        const int64_t e = q0 * k * std::max(ostride, 1);
        if (D) o.D += q0 * k;
        o.I += e;
        if (S64) o.S64 += e;
        if (cert) o.cert += q0;
        return o;
    }
};
// full_scan_block: gate = the fallback round's failure count (the launch returns at once while it
// is 0), or null = run; each workgroup's row range is at least rows_per_wg long; fallback: the
// scanned queries count in this call's counter or the index's (a first pass is counted nowhere);
// all_queries: scan every query of the block (cert is only written)
struct ScanOpts {
    const int* gate = nullptr;
    int rows_per_wg = TR;
    bool fallback = true;
    bool all_queries = false;
};
constexpr int kOptimisticSeedRank = 1;  // seed_rank argument: > 0 selects the optimistic rank
void health_poll(vs_index* ix);  // observe a completed failure-count readback (caller holds h_mu)
void full_scan_block(vs_index* ix, Ctx* c, const float* q, int nqb, int k, const SearchOut& out, hipStream_t st,
                     const ScanOpts& o);
// the sizing and the arguments the exact scans share: workgroups over a sequence of nseq rows (or
// list positions), at least len_per_wg each, at most wg_cap and what the scratch budget allows; the
// block's scratch and done counters; every FullScanArgs field but gate and count
FullScanArgs full_scan_args(vs_index* ix, Ctx* c, int64_t nseq, int len_per_wg, int64_t wg_cap, const float* q, int nqb,
                            int k, const SearchOut& out, bool all_queries, hipStream_t st);
void search_all(vs_index* ix, Ctx* c, const float* q, int64_t nq, int k, int Kp, const SearchOut& out, hipStream_t st,
                int seed_rank, bool device_fallback = false);
// the MFMA screen of a whole shard at depth MFMA_KP_MAX, one workgroup per CU at most (i8: over the
// int8 copy), and its workspace: candidate buffers, survivor lists, list counters and drop bounds
ScreenArgs mfma_screen_base(const vs_index* ix, bool i8);
void mfma_workspace(Ctx* c, ScreenArgs& a);
float xmax_of(const vs_index* ix);  // upper bound on ||x|| over the shard (RefineArgs::xmax)
void check_k(int k, int kmax = K_MAX);
// host entry points: queries and results pass through pinned staging of at most kPinnedStageCap
// bytes per context, in chunks of queries (whole MFMA batches when a chunk holds more than one)
int64_t stage_chunk(const vs_index* ix, int64_t nq, int kk, bool with_cert);
void stage_queries(const vs_index* ix, Ctx* c, const float* q, int64_t q0, int64_t m, hipStream_t st);
// a chunk's device and pinned host result blocks, one layout [I int64 | D fp32 | cert int] (exact_lists)
struct StagedOut {
    int64_t *Id, *Ik;
    float *Dd, *Dk;
    int *cert_d, *cert_h;
    size_t bytes;
    int64_t redo;  // exact_lists: the queries the selector's overfetch tier left short and its scan re-answered
};
float worst_score(const vs_index* ix);
void fill_padding(float* D, int64_t* I, int64_t n, float fillD);
// [m][kk] staged results -> the caller's [..][k] rows from q0 on, padded past kk (faiss layout)
void scatter_padded(const StagedOut& o, int64_t q0, int64_t m, int k, int kk, float fillD, float* D, int64_t* I);

// ---- vs_sel_host.hip ----
void check_sel(const vs_index* ix, const vs_sel* sel);
// the tier of one filtered call (vs_set_sel_mode, the AUTO rule) and its run over one batch of device
// queries: outputs device [nq][k]; returns the queries the overfetch tier left short and the scan
// re-answered; synchronises st on that tier.  sel_note_stats files what vs_sel_last_stats reports.
struct SelPlan {
    int tier;  // VS_SEL_SCAN / VS_SEL_OVERFETCH
    int kp;    // the overfetch depth k' (0 for the scan)
};
SelPlan sel_plan(const vs_index* ix, const vs_sel* sel, int64_t nq, int k);
int64_t sel_search_ctx(vs_index* ix, Ctx* c, const vs_sel* sel, const SelPlan& plan, const float* q, int64_t nq, int k,
                       const SearchOut& out, hipStream_t st);
void sel_note_stats(vs_index* ix, const vs_sel* sel, const SelPlan& plan, int64_t redo);

// vs_search.hip -- one road from a staged chunk to exact lists: the m queries in c->qdev ranked at depth
// kk over the members of sel (plan: its sel_plan for the call) or over every row (sel null) into the
// chunk's blocks, valid afterwards where want says: LISTS_HOST (Ik / Dk; the stream is waited for) and /
// or LISTS_DEVICE (Id / Dd: a kernel reads them).  The selector road's re-answered count is in redo.
enum : unsigned { LISTS_HOST = 1, LISTS_DEVICE = 2 };
StagedOut exact_lists(vs_index* ix, Ctx* c, const vs_sel* sel, const SelPlan& plan, int64_t m, int kk, unsigned want,
                      hipStream_t st);

// ---- vs_group_host.hip ----
void check_groups(const vs_index* ix, const vs_groups* gr);

// ---- vs_range_host.hip ----
struct RangeStats {
    int64_t total = 0, tier = VS_RANGE_SCAN, rescanned = 0, host_sorted = 0;
};
// queries taken from stored rows: the block's device array of row ids, VS_SELF_*, and (ABOVE without a
// selector) the smallest of those ids
struct RangeSelf {
    const int64_t* ids = nullptr;
    int mode = VS_SELF_KEEP;
    int64_t row0 = 0;
};
bool range_screen_applies(const vs_index* ix, const vs_sel* sel, int nqb);
// the SCREEN tier's first half over one block of device queries: the native MFMA screen of every stored
// row started at the key of radius_d[q] (device [nqb]); the survivors are in glist / gcnt of the result,
// its drop / thr0 say which lists a workgroup had to cut
ScreenArgs range_screen(vs_index* ix, Ctx* c, const float* qd, int nqb, const float* radius_d, hipStream_t st);
// One block of <= MFMA_QB device queries: counts[q] = the query's result count; unless count_only,
// its rows are appended to res (D, I, S) in query order, each query's best first.
void range_block(vs_index* ix, Ctx* c, const vs_sel* sel, const float* qd, int nqb, const float* rad, bool screen,
                 bool count_only, hipStream_t st, RangeStats& stt, int64_t* counts, vs_range_result* res,
                 const RangeSelf& self = RangeSelf());
void range_note_stats(vs_index* ix, const RangeStats& s);

}  // namespace vs

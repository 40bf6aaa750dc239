// vs_search.hip -- search orchestration of the flat index: screen health, the depth and union rules,
// the query-block passes (int8 and native screens, refines, the full scan), the exact device
// searches, the two-phase sharded step and the host-buffer search.
#include "vs_index.h"

using namespace vs;

namespace vs {

ScreenArgs mfma_screen_base(const vs_index* ix, bool i8) {
    const int64_t tiles = (ix->ntotal + TR - 1) / TR;
    ScreenArgs a{};
    a.corpus = i8 ? ix->data8 : ix->data;
    a.n_valid = ix->ntotal;
    a.tiles = (int)tiles;
    a.dpad = i8 ? ix->dpad8 : ix->dpad;
    a.d = ix->d;
    a.metric = ix->metric;
    a.sqn = ix->sqn;
    a.Kp = MFMA_KP_MAX;
    a.cap = MFMA_CAP;
    a.G = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, ix->num_cu));
    if (i8) a.rsb = ix->rsb;
    return a;
}

// (a.G, a.Kp and a.cap are final; the query pack zeroes the counters and bounds)
void mfma_workspace(Ctx* c, ScreenArgs& a) {
    a.lcap = a.G * a.Kp;
    c->gcnt.ensure(sizeof(int) * MFMA_QB);
    c->drop.ensure(sizeof(u64) * MFMA_QB);
    c->cand.ensure((size_t)a.G * MFMA_QB * a.cap * sizeof(u64));
    c->part.ensure((size_t)MFMA_QB * a.lcap * sizeof(u64));
    a.cand = c->cand.as<u64>();
    a.glist = c->part.as<u64>();
    a.gcnt = c->gcnt.as<int>();
    a.drop = c->drop.as<u64>();
}

float xmax_of(const vs_index* ix) { return (float)(std::sqrt((double)ix->maxsq) * (1.0 + 1e-5)) + 1e-30f; }

}  // namespace vs

namespace {

// optimistic seed: a 16-row-group maximum of the strided tile sample, at the rank that leaves
// ~kOptimisticPassFactor * Kp corpus rows above it in expectation (the proven seed is rank Kp); a
// query left short is caught by the certificate and searched again with the proven seed
constexpr double kOptimisticPassFactor = 8.0;
constexpr int kOptimisticMinRank = 4;

// the seed pass screens each main-pass workgroup's first tile and the (native) main pass reuses
// its accumulators; the GEMV screen takes tiles from a work queue over its resident blocks (both
// measured faster than the alternatives they replaced)
constexpr bool seed_reuse() { return true; }
constexpr bool gemv_dyn() { return true; }

// The int8 pre-screen serves first passes of MFMA-sized batches (k <= I8_MAX_K) of an index with
// VS_SCREEN_I8; a query its certificate rejects is re-searched by the caller on the native path.
bool use_i8(const vs_index* ix, int nqb, int k) {
    if (ix->screen != VS_SCREEN_I8 || nqb <= GEMV_NQ_MAX || k > I8_MAX_K) return false;
    if (!ix->i8_res) return true;
    // group-residual codes: only the seed pass and the direct main pass add <mu_g, q> (else: native)
    const int64_t tiles = (ix->ntotal + TR - 1) / TR;
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>(tiles, ix->num_cu));
    return tiles >= 4 * G;
}

constexpr int kF32MfmaMinQ = 64;     // fp32 native batches: MFMA screen from this many queries on
constexpr int kI8RouteBatches = 64;  // searches routed to the native screen after a failing int8 batch
constexpr int kSeedScaleMax = 6;     // native optimistic seed: at most 64x the default depth
constexpr int kSeedRelax = 64;       // clean native batches before the depth is halved again
constexpr int kI8ScaleMax = 4;       // int8 union: at most 16x its target before routing to native
constexpr int kI8RouteLog2Max = 6;   // routing stretches: at most 64 x kI8RouteBatches searches


}  // namespace

namespace vs {

// observe a completed failure-count readback (caller holds h_mu)
void health_poll(vs_index* ix) {
    if (ix->h_pending && hipEventQuery(ix->h_ev) == hipSuccess) {
        const unsigned f = *ix->h_fails;
        if (ix->h_pending == 1) {
            // an int8 batch with failures: a deeper union first (dense score distributions put
            // more rows inside the int8 error window), the native screen when even the deepest
            // union failed; clean batches relax the depth again
            // (a batch where over a quarter of the queries failed deepens two steps at once; each
            // routing that follows a failure at the deepest union lasts twice as long as the last,
            // up to 2^kI8RouteLog2Max times kI8RouteBatches, so a corpus the int8 window cannot
            // serve costs one failing batch per ever longer native stretch)
            if (f > 0) {
                if (ix->i8_log2 < kI8ScaleMax) {
                    ix->i8_log2 = std::min(kI8ScaleMax, ix->i8_log2 + (f > (unsigned)(ix->h_nq / 4) ? 2 : 1));
                } else {
                    ix->i8_route = kI8RouteBatches << ix->i8_route_log2;
                    ix->i8_route_log2 = std::min(ix->i8_route_log2 + 1, kI8RouteLog2Max);
                }
                ix->i8_clean = 0;
            } else {
                ix->i8_route_log2 = 0;
                if (ix->i8_log2 > 0 && ++ix->i8_clean >= kSeedRelax) {
                    --ix->i8_log2;
                    ix->i8_clean = 0;
                }
            }
        } else if (f > 0) {  // (one failed query costs its block a whole fallback screen: deepen)
            ix->seed_log2 = std::min(ix->seed_log2 + 1, kSeedScaleMax);
            ix->seed_clean = 0;
        } else if (ix->seed_log2 > 0 && ++ix->seed_clean >= kSeedRelax) {
            --ix->seed_log2;
            ix->seed_clean = 0;
        }
        ix->h_clean = f > 0 ? 0 : ix->h_clean + 1;
        ix->h_pending = 0;
    }
    (void)hipGetLastError();  // (hipEventQuery's "not ready" is no error)
}


}  // namespace vs

namespace {

// May this search use the int8 screen?  Consumes the routing state (one call per search).
bool i8_allowed(vs_index* ix) {
    if (ix->screen != VS_SCREEN_I8) return false;
    std::lock_guard<std::mutex> g(ix->h_mu);
    health_poll(ix);
    if (ix->i8_route > 0) {
        --ix->i8_route;
        return false;
    }
    return true;
}

// depth multiplier of the native optimistic seed
double seed_scale(vs_index* ix) {
    std::lock_guard<std::mutex> g(ix->h_mu);
    health_poll(ix);
    return (double)(1 << ix->seed_log2);
}

// after a first-pass batch (kind 1 int8, 2 native): read its failure count back behind it on the
// stream (one readback in flight per index)
// A long clean run reads back only every kHealthStride-th batch (a readback is a copy launch and ~10
// us of the 8-shard step); the first failing readback returns to every batch.
constexpr int kHealthCleanRun = 16;
constexpr unsigned kHealthStride = 4;

void health_note(vs_index* ix, Ctx* c, hipStream_t st, int kind, int nq) {
    std::lock_guard<std::mutex> g(ix->h_mu);
    if (ix->h_pending) return;
    if (ix->h_clean >= kHealthCleanRun && (++ix->h_seq % kHealthStride) != 0) return;
    if (!ix->h_fails) {
        HIP_CHECK(hipHostMalloc((void**)&ix->h_fails, sizeof(unsigned), hipHostMallocDefault));
        HIP_CHECK(hipEventCreateWithFlags(&ix->h_ev, hipEventDisableTiming));
    }
    HIP_CHECK(hipMemcpyAsync(ix->h_fails, c->fails.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(ix->h_ev, st));
    ix->h_pending = kind;
    ix->h_nq = nq;
}

// int8 GEMV screen depth.  Its keys carry the row error bound beta (~0.007-0.01 ||x|| ||q||), so the
// rows it must keep are those within ~beta of the k-th best.  For unit rows the scores are roughly
// N(0, 1/d) and the k-th best sits z = sqrt(2 ln(N / k)) deviations out, where the density grows by
// e^(z beta sqrt(d)) per beta: keep k times twice that (+64); deeper than kI8GemvMaxDepth, the
// native GEMV serves the query.  Data that defeat the estimate fail the certificate, not exactness.
// beta enters relative to max ||x||, so the depth does not depend on the rows' scale (as an absolute
// norm it sent every index of rows scaled by 2^12 to the native GEMV and cut one scaled by 2^-40
// to the minimum depth).
constexpr int kI8GemvMaxDepth = 512;

int i8_gemv_depth(const vs_index* ix, int k) {
    const double z = std::sqrt(2.0 * std::log(std::max(2.0, (double)ix->ntotal / k)));
    const double xm = std::sqrt((double)ix->maxsq);
    const double beta = xm > 0.0 ? (double)ix->i8_bmax / xm : 0.0;
    const double g = std::exp(std::min(20.0, z * beta * std::sqrt((double)ix->d)));
    return (int)std::min<double>(KP_MAX, round_up((int64_t)std::ceil(2.0 * k * g + 64.0), 16));
}

// Union of survivors the int8 seed aims at (rows above the seeded threshold).  It must cover the
// refine's window -- every key within the int8 error budget of T', measured at ~7.5-10 k rows for
// unit-norm data -- or the certificate fails and the query is re-searched.  The seed is
// the rank-r maximum over S sampled rows, r = U S / N, so the count above it is U (1 +- ~1/sqrt r):
// take the smallest U whose 3-sigma low count still covers kI8Window * k rows, within
// [kI8UnionMin, kI8UnionMaxPerK * k].  Large shards need more margin (few sampled maxima per union
// row): cfg3's 10M rows -> ~41 k, the 8-GPU shard of 1.25M rows -> ~25 k (union sweep).
constexpr double kI8Window = 15.0;
constexpr double kI8UnionMaxPerK = 64.0;
constexpr double kI8UnionMin = 1024.0;

double i8_union_target(int k, double sampled, double n) {
    const double need = kI8Window * k;
    double u = std::max(need, kI8UnionMin);
    const double umax = std::max(kI8UnionMaxPerK * k, kI8UnionMin);
    while (u < umax) {
        const double r = u * sampled / n;
        if (r >= 9.0 && u * (1.0 - 3.0 / std::sqrt(r)) >= need) break;
        u *= 1.1;
    }
    return std::min(u, umax);
}

// the events around a timed screen launch (vs_set_timing): started at construction, stop(kind) files
// the pair for vs_timing_fetch
struct ScreenTimer {
    vs_index* ix;
    hipStream_t st;
    bool on;
    DevEvent e0, e1;
    ScreenTimer(vs_index* ix_, hipStream_t st_, bool enable = true) : ix(ix_), st(st_), on(enable && ix_->timing.load()) {
        if (!on) return;
        e0.create();
        e1.create();
        HIP_CHECK(hipEventRecord(e0, st));
    }
    void stop(int kind) {
        if (!on) return;
        HIP_CHECK(hipEventRecord(e1, st));
        std::lock_guard<std::mutex> g(ix->tmtx);
        ix->tev.emplace_back(std::move(e0), std::move(e1));
        ix->last_kernel_kind = kind;
    }
};

// the RefineArgs fields both refines fill alike: the block's queries, the stored rows, the outputs
RefineArgs refine_base(const vs_index* ix, const float* q, const SearchOut& out, int k) {
    RefineArgs r{};
    r.q = q;
    r.d = ix->d;
    r.dpad = ix->dpad;
    r.dt = ix->dtype;
    r.metric = ix->metric;
    r.corpus = ix->data;
    r.xmax = xmax_of(ix);
    r.k = k;
    r.n_valid = ix->ntotal;
    r.id_offset = out.id_offset;
    r.D = out.D;
    r.I = out.I;
    r.S64 = out.S64;
    r.cert = out.cert;
    r.ostride = out.ostride;
    r.rows = (unsigned long long*)(ix->d_maxsq + IX_REFINE_ROWS);
    return r;
}

// Threshold seeding of an MFMA main pass `a` (>= 4 tiles per workgroup): screen one tile per
// workgroup, strided over the shard, keep only the per-query maxima of 16-row groups, and start every
// workgroup of the main pass at the rank-th largest of them, rank = rank_of(sampled rows, maxima
// per query).  Sets a.thr0 (and a.seed_acc) and returns the rank.
// direct: the main pass screens its whole range itself; otherwise the seed tile is the first tile
// of each main-pass workgroup and its raw accumulators are kept, so the main pass starts one tile later
template <typename RankOf>
int seed_pass(vs_index* ix, Ctx* c, ScreenArgs& a, int dt, bool direct, int nqb, hipStream_t st, RankOf rank_of) {
    ScreenArgs sa = a;
    sa.G = std::min(sa.G, 512);  // k_seed_select holds up to 8192 maxima per query
    sa.tile_stride = a.tiles / sa.G;
    if (seed_reuse() && sa.G == a.G && !direct) {
        c->seedacc.ensure((size_t)a.G * 128 * MF_WG_THREADS * sizeof(float));
        sa.seed_acc = c->seedacc.as<float>();
    }
    const int M = sa.G * 16;
    c->seedmax.ensure(sizeof(float) * MFMA_QB * M);
    sa.seedmax = c->seedmax.as<float>();
    HIP_CHECK(launch_seed_mfma(dt, sa, c->qtile.as<uint8_t>(), nqb, st));
    c->thr0.ensure(sizeof(u64) * MFMA_QB);
    const int rank = rank_of((double)sa.G * TR, M);
    HIP_CHECK(launch_seed_select(sa.seedmax, M, nqb, rank, c->thr0.as<u64>(), st));
    a.thr0 = c->thr0.as<u64>();
    a.seed_acc = sa.seed_acc;
    return rank;
}

struct I8Opts {
    int phase = 0, ka = 0;         // phase 1: stop after a refine phase A of ka keys ...
    RefineArgs* keep = nullptr;    // ... and leave the refine's arguments here
    int kwin = 0;                  // > 0: the seed's union covers this k instead of k
    bool prepack = false;          // a device fallback round follows: pack its native tile too
};
// int8 pre-screen of one query block: pack int8 query codes -> seed pass -> int8 MFMA screen with
// upper-bound keys -> adaptive exact refine (k_refine_wide).  q: device fp32 [nqb][d].
// phase 1 (two-phase sharded search, o.ka keys in phase A): stops after the refine's phase A and
// returns its arguments in *o.keep for vs_search_device_phase_b
void search_block_i8(vs_index* ix, Ctx* c, const float* q, int nqb, int k, const SearchOut& out, hipStream_t st,
                     const I8Opts& o = I8Opts()) {
    // (L2: keys 2 (upper bound of <x, q>) - ||x||^2; Kp is per workgroup and query, the refine's
    // depth is adaptive)
    ScreenArgs a = mfma_screen_base(ix, true);
    const int64_t tiles = a.tiles;
    c->qtile.ensure((size_t)MFMA_QB * ix->dpad8);
    c->qfac.ensure(sizeof(float2) * MFMA_QB);
    c->qeps.ensure(sizeof(float) * MFMA_QB);
    mfma_workspace(c, a);
    c->fails.ensure(2 * sizeof(int));
    // threshold seeding: a seed pass + select before the main pass (>= 4 tiles per workgroup).
    // (Round 4 measured the alternative -- each workgroup of the direct main pass screening a sample
    // tile first and the workgroups selecting and adopting the seed among themselves, no extra
    // launches -- on MI355X: 0.19-0.23 ms slower per cfg3 batch (K1 3.96 vs 3.73 ms) and 0.2 ms at
    // the 8-shard's 1.25M rows, the tiles screened under provisional thresholds costing more than
    // the two launches, profiles/r04_seed_ab.txt; it was removed.)
    const bool seeded = tiles >= 4 * (int64_t)a.G;
    if (ix->i8_res && !(seeded && ix->metric == METRIC_IP && i8_direct_ok(ix->dpad8)))
        throw VsError(VS_ERR_INTERNAL, "group-residual int8 codes need the seeded direct pass");
    if (ix->i8_res) {  // <mu_g, q> of every group for this block's queries
        const int64_t ng = (ix->ntotal + I8_GROUP_ROWS - 1) / I8_GROUP_ROWS;
        c->gT.ensure((size_t)ng * MFMA_QB * sizeof(float));
        HIP_CHECK(launch_group_dots(ix->gmean, ng, ix->dpad8, q, nqb, ix->d, c->gT.as<float>(), st));
        a.gT = c->gT.as<float>();
    }
    // (a device fallback round follows: its native tile is packed here too, from the same loads)
    NativeTile nat{};
    c->prepacked = 0;
    if (o.prepack && (ix->dtype == DT_BF16 || ix->dtype == DT_F16)) {
        c->qtile_n.ensure((size_t)MFMA_QB * ix->dpad * ix->es);
        c->qinfo.ensure(sizeof(float) * 2 * MFMA_QB);
        c->gcnt2.ensure(sizeof(int) * MFMA_QB);
        c->drop2.ensure(sizeof(u64) * MFMA_QB);
        nat = NativeTile{ix->dtype, (int)ix->dpad, c->qtile_n.as<uint8_t>(), c->qinfo.as<float>(), c->gcnt2.as<int>(),
                         c->drop2.as<u64>()};
    }
    HIP_CHECK(launch_pack_qtile_i8(q, nqb, ix->d, ix->dpad8, c->qtile.as<uint8_t>(), c->qfac.as<float2>(),
                                   c->qeps.as<float>(), ix->d_maxsq + 2, c->gcnt.as<int>(), c->drop.as<u64>(), st,
                                   c->fails.as<int>(), ix->metric == METRIC_L2 ? ix->d_maxsq : nullptr,
                                   gamma_of(ix->d), nat.qt ? &nat : nullptr));
    if (nat.qt) c->prepacked = 2;
    a.qfac = c->qfac.as<float2>();
    if (seeded) {  // optimistic threshold seed from one tile per workgroup
        // (the direct main pass, k_screen_i8d, screens its whole range itself; the other form reuses
        // the seed tile's accumulators)
        seed_pass(ix, c, a, DT_I8, i8_direct_ok(ix->dpad8), nqb, st, [&](double sampled, int M) {
            double target = i8_union_target(o.kwin > 0 ? o.kwin : k, sampled, (double)ix->ntotal);
            {
                std::lock_guard<std::mutex> g(ix->h_mu);
                target *= (double)(1 << ix->i8_log2);
            }
            const double r = std::ceil(target * sampled / (double)ix->ntotal);
            return (int)std::min<double>(std::max<double>(r, (double)kOptimisticMinRank), (double)M);
        });
    }
    ScreenTimer timer(ix, st);
    HIP_CHECK(launch_screen_mfma(DT_I8, a, c->qtile.as<uint8_t>(), nqb, st));
    timer.stop(3);
    RefineArgs r = refine_base(ix, q, out, k);
    r.cand = a.glist;
    r.cand_n = a.gcnt;
    r.lcap = a.lcap;
    r.Kp = a.Kp;
    r.uncert = ix->d_uncert;
    r.qeps = c->qeps.as<float>();
    r.drop = a.drop;
    r.thr0 = a.thr0;
    r.fails = c->fails.as<int>();
    if (o.phase == 1) {
        const int ka = o.ka;
        const int kah = rfw_ka_hi(ka);  // (phase A keeps up to this many rows per query)
        c->pa.ensure((size_t)nqb * kah * 12 + (size_t)nqb * 16);
        r.phase = 1;
        r.pa_cap = kah;
        r.pa_sc = c->pa.as<double>();
        r.pa_ids = (uint32_t*)(r.pa_sc + (size_t)nqb * kah);
        r.pa_tA = (u64*)(r.pa_ids + (size_t)nqb * kah);
        r.pa_n = (int*)(r.pa_tA + nqb);
        HIP_CHECK(launch_refine_wide(r, nqb, ka, st));
        if (o.keep) *o.keep = r;
        return;
    }
    // (phase-A depths just under a power of two: the phase-A selection may stop anywhere up to
    // that power -- rfw_ka_hi -- instead of bisecting to an exact count)
    HIP_CHECK(launch_refine_wide(r, nqb, (int)round_up(2 * k + 24, 8), st));
}

// Enqueue one query block through screen -> merge -> refine.  q: device fp32 [nqb][d].
// seed_rank: 0 = proven (safe) seed, > 0 = optimistic seed at that sample rank (see k_seed_select)
// redo: the device fallback round of the block just searched (MFMA dtypes, unseeded screen): its
// three launches (pack, screen, refine) are gated on the block's failure count (c->fails) and the
// refine rewrites only the queries whose certificate failed; a query it cannot certify either
// counts in c->fails[1], the gate of the block's full scan (full_scan_block)
// allow_i8: the int8 pre-screen may serve the block (first passes of an index with that screen)
// prepack (first passes followed by their device fallback round): the round's native query tile
// and zeroed list counters are prepared by this pass's query pack (Ctx::prepacked)
struct BlockOpts {
    int seed_rank = 0;
    bool redo = false, allow_i8 = true, prepack = false;
};
void search_block(vs_index* ix, Ctx* c, const float* q, int nqb, int k, int Kp, const SearchOut& out, hipStream_t st,
                  const BlockOpts& o) {
    const int seed_rank = o.seed_rank;
    const bool redo = o.redo;
    if (!redo) c->prepacked = 0;
    if (seed_rank > 0 && o.allow_i8 && use_i8(ix, nqb, k)) {
        I8Opts i8;
        i8.prepack = o.prepack;
        search_block_i8(ix, c, q, nqb, k, out, st, i8);
        health_note(ix, c, st, 1, nqb);
        return;
    }
    // (search_all makes blocks of > GEMV_NQ_MAX queries only where the MFMA screen serves them)
    const bool use_mfma = nqb > GEMV_NQ_MAX || redo;
    const int* gate = redo ? c->fails.as<int>() : nullptr;
    if (!redo) c->fails.ensure(2 * sizeof(int));
    // int8 screen, few queries: the GEMV streams the int8 copy (1 B per element) with the fp32
    // query; its keys carry the row error bound, so it screens deeper (first passes only)
    bool gemv_i8 = !use_mfma && seed_rank > 0 && ix->screen == VS_SCREEN_I8 && ix->data8 != nullptr && !ix->i8_res;
    if (gemv_i8) {
        const int kp8 = i8_gemv_depth(ix, k);
        gemv_i8 = kp8 <= kI8GemvMaxDepth;  // a single query's refine is one workgroup: deep lists cost
        if (gemv_i8) Kp = kp8;             // more than the int8 stream saves -> native GEMV
    }
    // (the GEMV screen reads the same rows: its depth, slots and grid are set below)
    ScreenArgs a = mfma_screen_base(ix, false);
    const int64_t tiles = a.tiles;
    // MFMA: each workgroup keeps its best min(Kp, MFMA_KP_MAX) per query; deeper screens certify
    // against the workgroups' compaction bounds (drop) in the refine.  First passes of inner-product
    // batches (adaptive refine below) keep MFMA_KP_MAX: a workgroup that holds many of a query's
    // best rows (a cluster inserted contiguously) then drops only rows far below the k-th best.
    // (the device fallback round too: its fixed-depth certificate needs two margins between the
    // k-th and the KP_MAX-th best, which a tight cluster -- scores denser than the bf16 query
    // rounding -- does not leave; the adaptive refine scores the rows inside one margin instead)
    const bool wide = use_mfma && ix->metric == METRIC_IP && k <= I8_MAX_K &&
                      (redo || refine_split(nqb, Kp, ix->dtype, ix->num_cu) <= 1);
    // (unseeded small shards -- under 4 tiles per workgroup -- keep max(128, 2 Kp) per workgroup:
    // MFMA_KP_MAX lists of every row there made the refine's selection the cost, 0.9 ms at 100k x
    // 4096 bf16, batch 256, k = 10; a workgroup holding more of a query's best rows fails its
    // certificate and the fallback round lists every row)
    const bool small_shard = tiles < 4 * (int64_t)ix->num_cu;
    a.Kp = use_mfma ? (wide ? (small_shard ? std::min(MFMA_KP_MAX, std::max(128, 2 * Kp)) : MFMA_KP_MAX)
                            : std::min(Kp, MFMA_KP_MAX))
                    : Kp;
    int QB;
    c->qinfo.ensure(sizeof(float) * 2 * MFMA_QB);
    // the screen's query tile and survivor-list counters (a fallback round prepared by its first pass:
    // the prepacked tile, counters gcnt2 / drop2, no pack launch)
    const int pre = redo ? c->prepacked : 0;
    c->prepacked = 0;
    const uint8_t* qtile = c->qtile.as<uint8_t>();
    int* gcnt = nullptr;
    u64* dropb = nullptr;
    if (use_mfma) {
        QB = MFMA_QB;
        c->qtile.ensure((size_t)MFMA_QB * ix->dpad * ix->es);
        mfma_workspace(c, a);
        a.part = a.glist;
        qtile = c->qtile.as<uint8_t>();
        gcnt = a.gcnt;
        dropb = a.drop;
        if (pre) {
            if (pre == 2) qtile = c->qtile_n.as<uint8_t>();
            gcnt = c->gcnt2.as<int>();
            dropb = c->drop2.as<u64>();
        } else {
            // a first pass whose fallback round follows zeroes that round's counters too
            const bool pp = o.prepack && !redo;
            if (pp) {
                c->gcnt2.ensure(sizeof(int) * MFMA_QB);
                c->drop2.ensure(sizeof(u64) * MFMA_QB);
            }
            HIP_CHECK(launch_pack_qtile(ix->dtype, q, nqb, ix->d, ix->dpad, c->qtile.as<uint8_t>(),
                                        c->qinfo.as<float>(), gcnt, dropb, st, redo ? nullptr : c->fails.as<int>(),
                                        gate, nullptr, pp ? c->gcnt2.as<int>() : nullptr,
                                        pp ? c->drop2.as<u64>() : nullptr));
            if (pp) c->prepacked = 1;
        }
    } else {
        QB = nqb <= 1 ? 1 : nqb <= 2 ? 2 : nqb <= 4 ? 4 : 8;
        a.cap = (int)round_up(Kp + 2 * TR, 256);
        const int sdt = gemv_i8 ? DT_I8 : ix->dtype;
        const int dpadq = gemv_i8 ? ix->dpad8 : ix->dpad;
        // work-queue tiles over exactly the resident blocks; a corpus of at most num_cu / 2 tiles
        // (cfg1: 40) would leave most CUs idle: its work items are quarter tiles (GEMV_SPLIT)
        const int64_t resident = (int64_t)ix->num_cu * (gemv_dyn() ? gemv_blocks_per_cu(sdt, QB, dpadq) : 8);
        a.gemv_split = tiles <= ix->num_cu / 2 ? GEMV_SPLIT : 1;
        a.G = (int)std::min<int64_t>(tiles * a.gemv_split, resident);
        // one query: each block keeps only Kb < Kp keys and publishes the key below which it dropped
        // rows (ScreenArgs::drop, the refine's certificate bound for them), so the G lists together
        // hold at most kRefineRegKeys keys -- the refine selects the best Kp from them in registers
        // and no k_merge launch runs (cfg2: 1024 blocks x 176 keys took a merge of 15 us).  A block
        // that drops a row the query needs fails the certificate; with ~Kp / G of the best rows per
        // block and Kb >= 16 that does not happen in practice.  First passes only (seed_rank > 0):
        // Kb does not grow with Kp, so the host API's 4x-deeper re-searches of a failed query (a
        // burst of near-duplicates in one block) keep whole Kp-deep lists and can certify it.
        if (nqb == 1 && seed_rank > 0 && ix->ntotal >= Kp) {
            const int kb = (int)std::max<int64_t>(16, (kRefineRegKeys / std::max(a.G, 1)) / 16 * 16);
            if (kb < Kp && (int64_t)a.G * kb <= kRefineRegKeys) {
                a.Kp = kb;
                a.cap = (int)round_up(kb + 2 * TR, 256);
                c->drop.ensure(sizeof(u64) * MFMA_QB);
                a.drop = c->drop.as<u64>();
            }
        }
        c->qpad.ensure((size_t)QB * dpadq * sizeof(float));
        int* ctr = nullptr;
        if (gemv_dyn()) {  // the work-queue counter is zeroed by the query pack (no separate memset)
            c->tilectr.ensure(sizeof(int));
            ctr = c->tilectr.as<int>();
        }
        HIP_CHECK(launch_pack_qf32(q, nqb, QB, ix->d, dpadq, c->qpad.as<float>(), c->qinfo.as<float>(), st, ctr,
                                   c->fails.as<int>(), a.drop));
        if (gemv_i8) {
            a.corpus = ix->data8;
            a.dpad = ix->dpad8;
            a.rsb = ix->rsb;
            a.qinfo = c->qinfo.as<float>();
        }
    }
    a.gate = gate;
    if (use_mfma) {
        if (redo) a.skip = out.cert;  // the fallback screens only the block's failed queries
        a.gcnt = gcnt;
        a.drop = dropb;
    } else {
        a.G = std::max(a.G, 1);
        c->cand.ensure((size_t)a.G * QB * a.cap * sizeof(u64));
        c->part.ensure((size_t)a.G * QB * a.Kp * sizeof(u64));  // [G][QB][Kp] per-block lists
        a.cand = c->cand.as<u64>();
        a.part = c->part.as<u64>();
        if (gemv_dyn()) a.next_tile = c->tilectr.as<int>();
    }

    // merge partial lists [nseg][qstride][Kp] down to one list per query (or, with stop_keys, to
    // the first round whose nseg * Kp <= stop_keys: one query's lists are then contiguous and the
    // refine selects the best Kp itself); returns it, nseg updated
    // (segments of a.Kp keys: the screen's per-block depth, = Kp whenever a merge runs)
    auto merge_all = [&](const u64* src, int& nseg, int qstride, int stop_keys) -> const u64* {
        const int W = a.Kp;
        const int spb = (256 * (W > 2048 ? 32 : 16)) / W;  // k_merge: 4096 / 8192 keys per block
        const size_t mbytes = (size_t)std::max(1, (nseg + spb - 1) / spb) * nqb * W * sizeof(u64);
        c->merge_a.ensure(mbytes);
        c->merge_b.ensure(mbytes);
        u64* bufs[2] = {c->merge_a.as<u64>(), c->merge_b.as<u64>()};
        int which = 0;
        while (nseg > 1 && (int64_t)nseg * W > stop_keys) {
            int nout = 0;
            HIP_CHECK(launch_merge(src, nseg, qstride, nqb, W, bufs[which], &nout, st));
            src = bufs[which];
            which ^= 1;
            nseg = nout;
            qstride = nqb;
        }
        return src;
    };

    // threshold seeding (MFMA path, seed_pass): rank = Kp is a proven lower bound, kOptimisticSeedRank
    // asks for the optimistic rank
    bool optimistic = false;
    // (not in a fallback round: its launches cost their dispatch on every call, and it rarely runs)
    if (use_mfma && !redo && tiles >= 4 * (int64_t)a.G) {
        // (bf16 / f16 main passes in the direct form screen their whole range themselves)
        const bool direct = (ix->dtype == DT_BF16 || ix->dtype == DT_F16) && d16_direct_ok(ix->dpad);
        const int rank = seed_pass(ix, c, a, ix->dtype, direct, nqb, st, [&](double sampled, int M) {
            if (seed_rank <= 0) return Kp;
            // optimistic rank: expected rows above the seed ~ rank * rows / sampled rows ~ 8 Kp
            // deep screens aim lower (~12k listed rows per query), so the refine selects in registers
            const double factor = std::min(kOptimisticPassFactor, 12288.0 / Kp) * (wide ? seed_scale(ix) : 1.0);
            const double r = std::ceil(factor * Kp * sampled / (double)ix->ntotal);
            // floor: at rank 1 a sample maximum that falls inside the true top-Kp leaves fewer than
            // Kp survivors (probability ~Kp * sampled / N per query, ~2% at 100M rows); with >= 4
            // sampled rows required in the top-Kp the failure odds drop to ~(that)^4 / 24
            // (the fixed-depth refine needs rank <= Kp -- the proven seed -- for its certificate; the
            // adaptive refine's certificate checks the seed itself, so its rank may go deeper)
            return (int)std::min<double>(std::max<double>(r, (double)kOptimisticMinRank), wide ? (double)M : (double)Kp);
        });
        optimistic = rank < Kp;
    }

    ScreenTimer timer(ix, st, !redo);  // (a fallback round is not the timed screen)
    if (use_mfma) HIP_CHECK(launch_screen_mfma(ix->dtype, a, qtile, nqb, st));
    else HIP_CHECK(launch_screen_gemv(gemv_i8 ? DT_I8 : ix->dtype, a, c->qpad.as<float>(), nqb, QB, st));
    timer.stop(use_mfma ? 1 : gemv_i8 ? 4 : 2);
    RefineArgs r = refine_base(ix, q, out, k);
    if (use_mfma) {  // the refine selects the best Kp of each query's survivor list itself
        r.cand = a.glist;
        r.cand_n = a.gcnt;
        r.lcap = a.lcap;
    } else {  // GEMV: merge the per-block lists down to [q][Kp] (qstride nqb, or part[0] with QB)
        // one query (the product's call shape): stop the merge tree at <= kRefineRegKeys keys,
        // which the refine selects from in registers (one wave up to 2048; a k_merge launch costs
        // more than the block-wide selection above that).  Needs >= Kp non-empty keys among them,
        // which every round keeps when the shard has >= Kp rows.
        int nseg = a.G;
        const int stop = (nqb == 1 && ix->ntotal >= Kp) ? kRefineRegKeys : 0;
        r.cand = merge_all(a.part, nseg, QB, stop);
        r.cand_n = nullptr;
        r.lcap = nseg * a.Kp;
    }
    r.Kp = Kp;
    r.drop = a.drop;
    r.thr0 = a.thr0;  // (the adaptive refine's certificate: rows never listed scored <= thr0)
    r.i8max = gemv_i8 ? ix->d_maxsq + 2 : nullptr;
    r.qinfo = c->qinfo.as<float>();
    r.gamma = gamma_of(ix->d);
    r.uncert = redo ? nullptr : ix->d_uncert;
    r.fails = c->fails.as<int>() + (redo ? 1 : 0);  // (a fallback round's failures gate the full scan)
    r.redo = redo ? 1 : 0;
    r.gate = gate;
    r.optimistic = optimistic ? 1 : 0;
    r.nsplit = redo ? 1 : refine_split(nqb, Kp, ix->dtype, ix->num_cu);
    if (r.nsplit > 1) {
        const int KP2 = refine_kp2(Kp);
        c->rsc.ensure((size_t)nqb * KP2 * 12);
        r.gsc = c->rsc.as<double>();
        r.gids = (uint32_t*)(r.gsc + (size_t)nqb * KP2);
        if (c->rdone.bytes < sizeof(unsigned) * MFMA_QB) {  // zeroed once; the last workgroup re-zeroes
            c->rdone.ensure(sizeof(unsigned) * MFMA_QB);
            HIP_CHECK(hipMemsetAsync(c->rdone.p, 0, c->rdone.bytes, st));
        }
        r.gdone = c->rdone.as<unsigned>();
    }
    // native MFMA first passes (inner product): the adaptive two-phase refine -- it scores every
    // listed row whose key is within the screen's margin of the k-th best, so dense score
    // distributions (clustered corpora) certify without a re-search; the fixed-depth refine's
    // certificate needs a gap of 2 margins between the k-th and the Kp-th best
    if (wide) {
        const int ka = redo ? screen_depth(k) : Kp;  // (a fallback round's Kp is the listing depth)
        HIP_CHECK(launch_refine_wide(r, nqb, (int)round_up(std::max(ka - 8, k + 24), 8), st));
        if (!redo) health_note(ix, c, st, 2, nqb);
        return;
    }
    HIP_CHECK(launch_refine(r, nqb, st));
}

// Depth of the device fallback round: the end of vs_search's host escalation (KP_MAX), within
// the shard.
int fallback_depth(const vs_index* ix) { return (int)std::min<int64_t>(KP_MAX, round_up(ix->ntotal, 16)); }


}  // namespace

namespace vs {

constexpr int64_t kFullScanScratchMax = 512ll << 20;
constexpr int64_t kFullScanScratch = 32ll << 20;  // per-workgroup lists of one block, at most
FullScanArgs full_scan_args(vs_index* ix, Ctx* c, int64_t nseq, int len_per_wg, int64_t wg_cap, const float* q, int nqb,
                            int k, const SearchOut& out, bool all_queries, hipStream_t st) {
    const int64_t ranges = (nseq + len_per_wg - 1) / len_per_wg;
    const int64_t per_wg = (int64_t)nqb * k * 12;
    // scratch: per workgroup one k-list per query of the block.  32 MiB serves ~100 workgroups at
    // 256 queries x k 100; deep lists (k in the thousands) may take up to kFullScanScratchMax so the
    // scan still reaches a quarter of the CUs (at 32 MiB, k = 3276 left it 3 workgroups)
    const int64_t budget = std::max<int64_t>(kFullScanScratch, std::min<int64_t>(kFullScanScratchMax,
                                                                                 per_wg * (ix->num_cu / 4)));
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(wg_cap, ranges), budget / per_wg));
    c->fsc.ensure(full_scan_scratch_bytes(nqb, G, k));
    if (c->fdone.bytes < sizeof(unsigned) * MFMA_QB) {  // zeroed once; each query's last workgroup re-zeroes
        c->fdone.ensure(sizeof(unsigned) * MFMA_QB);
        HIP_CHECK(hipMemsetAsync(c->fdone.p, 0, c->fdone.bytes, st));
    }
    FullScanArgs a{};
    a.corpus = ix->data;
    a.d = ix->d;
    a.dpad = ix->dpad;
    a.dt = ix->dtype;
    a.metric = ix->metric;
    a.n_valid = ix->ntotal;
    a.q = q;
    a.nq = nqb;
    a.k = k;
    a.cert = out.cert;
    a.id_offset = out.id_offset;
    a.D = out.D;
    a.I = out.I;
    a.S64 = out.S64;
    a.ostride = out.ostride;
    a.gsc = c->fsc.as<double>();
    a.gid = (uint32_t*)(a.gsc + (size_t)nqb * G * k);
    a.gdone = c->fdone.as<unsigned>();
    a.G = G;
    a.all_queries = all_queries ? 1 : 0;
    return a;
}

// The last tier: an exact full scan of the shard (vs_fullscan.hip) for the block's queries with
// cert[q] == 0 -- those no bounded screen could certify (more rows than KP_MAX tied within its
// margin, e.g. thousands of identical embeddings).  Every row is scored canonically and streamed
// through a running top-k, so the answer is faiss's (ties to the lowest ids) for any tie count.
// gate: the fallback round's failure count (c->fails[1]; the launch returns at once while it is
// 0), or null = run.  Scanned queries count in this call's counter or the index's d_unres.
void full_scan_block(vs_index* ix, Ctx* c, const float* q, int nqb, int k, const SearchOut& out, hipStream_t st,
                     const ScanOpts& o) {
    FullScanArgs a = full_scan_args(ix, c, ix->ntotal, o.rows_per_wg, ix->num_cu, q, nqb, k, out, o.all_queries, st);
    a.gate = o.gate;
    a.count = !o.fallback ? nullptr : c->unres ? c->unres : ix->d_unres;  // (a first pass is counted nowhere)
    HIP_CHECK(launch_full_scan(a, st));
}

// Full search of nq device queries; outputs device [nq][k].  device_fallback: every block's first
// pass is followed by its gated fallback round (no host round trip; MFMA dtypes only).
// (measured against the GEMV screen + refine, scripts/small_scan_timing.py: the scan wins up to
// ~190 MB at d >= 1536 and k = 10; more rows, smaller d or deeper k favour the screen)
constexpr int kSmallScanQ = 2;           // queries per call
constexpr int kSmallScanMaxK = 64;
constexpr int64_t kSmallScanMaxRows = 65536;
constexpr int kSmallScanRows = 64;       // rows per workgroup range

bool small_scan(const vs_index* ix, int64_t nq, int k) {
    return nq <= kSmallScanQ && k <= kSmallScanMaxK && ix->ntotal <= kSmallScanMaxRows &&
           (int64_t)ix->ntotal * ix->dpad * ix->es <= ix->scan_limit.load();
}


}  // namespace

namespace vs {

void search_all(vs_index* ix, Ctx* c, const float* q, int64_t nq, int k, int Kp, const SearchOut& out, hipStream_t st,
                int seed_rank, bool device_fallback) {
    // One or two queries over a small corpus (the product's single-query call, BASELINE cfg1): the
    // exact full scan alone -- every row scored canonically in one launch, no screen, no refine, no
    // certificate to fail (measured: DESIGN §5 "Small corpora").  First passes only (seed_rank > 0):
    // a re-search of a certificate failure never reaches here, since this path has none.
    if (seed_rank > 0 && small_scan(ix, nq, k)) {
        SearchOut o = out;
        if (!o.cert) {
            c->cert.ensure((size_t)nq * sizeof(int));
            o.cert = c->cert.as<int>();
        }
        ScanOpts so;
        so.rows_per_wg = kSmallScanRows;
        so.fallback = false;
        so.all_queries = true;
        ScreenTimer timer(ix, st);
        full_scan_block(ix, c, q, (int)nq, k, o, st, so);
        timer.stop(5);
        return;
    }
    const bool i8 = seed_rank > 0 && i8_allowed(ix);  // (int8 screen on, and not routed away)
    const bool mfma_ok = (i8 && k <= I8_MAX_K) || ix->dtype != DT_F32;
    int64_t done = 0;
    while (done < nq) {
        const int64_t rem = nq - done;
        int nqb;
        // fp32 rows on the native screen: the fp32 MFMA (compute-bound, all 256 columns) pays from
        // ~kF32MfmaMinQ queries on; fewer take the GEMV, 8 queries per corpus pass
        if ((mfma_ok && rem > GEMV_NQ_MAX) || (!i8 && ix->dtype == DT_F32 && rem >= kF32MfmaMinQ))
            nqb = (int)std::min<int64_t>(rem, MFMA_QB);
        else nqb = (int)std::min<int64_t>(rem, GEMV_NQ_MAX);
        const float* qb = q + done * ix->d;
        const SearchOut ob = out.at(done, k);
        BlockOpts first;
        first.seed_rank = seed_rank;
        first.allow_i8 = i8;
        first.prepack = device_fallback && nqb > GEMV_NQ_MAX;
        search_block(ix, c, qb, nqb, k, Kp, ob, st, first);
        ScanOpts scan;
        if (device_fallback && nqb <= GEMV_NQ_MAX) {
            // a GEMV block (1-8 queries): a failed certificate goes straight to the full scan -- one
            // pass over the rows per failed query, about what the fallback round's MFMA screen costs
            // the block -- in ONE gated launch instead of four (the single-query step, cfg2)
            scan.gate = c->fails.as<int>();
            full_scan_block(ix, c, qb, nqb, k, ob, st, scan);
        } else if (device_fallback) {
            BlockOpts redo;
            redo.redo = true;
            search_block(ix, c, qb, nqb, k, std::max(Kp, fallback_depth(ix)), ob, st, redo);
            scan.gate = c->fails.as<int>() + 1;
            full_scan_block(ix, c, qb, nqb, k, ob, st, scan);
        }
        done += nqb;
    }
}


}  // namespace vs

// exact device search (vs_search_device_exact; the IVF coarse quantizer): like vs_search_device,
// but certificate failures are re-searched on the device, by each query block's gated fallback
// round at the deepest screen (KP_MAX, where vs_search's escalation ends; fp32 rows: the fp32 MFMA
// screen), and a query even that round cannot certify by the gated exact full scan of the shard
// (full_scan_block; counted in vs_full_scan_count).  async: no host round trip at all, the call
// returns with the work queued; otherwise the certificates are read back and checked.
void vs::search_exact_device(vs_index* ix, const float* q_dev, int64_t nq, int k, int64_t* I_dev, double* S64_dev,
                             hipStream_t st, float* D_dev, int64_t id_offset, bool async, unsigned* unres) {
    check_index(ix);
    if (nq <= 0) return;
    std::shared_lock<std::shared_mutex> lk(ix->rw);
    DeviceGuard dg(ix->device);
    if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");  // k > ntotal: -1 / worst-score padding
    CtxLease L(ix, st, false);
    Ctx* c = L.c;
    c->outD.ensure((size_t)nq * k * sizeof(float));
    c->cert.ensure((size_t)nq * sizeof(int));
    const int Kp = screen_depth(k);
    UnresScope us(c, unres);  // the caller's counter for this call only (the Ctx goes back to the pool)
    // every dtype has the on-device MFMA fallback round, queued behind each block's first pass
    const SearchOut out{D_dev ? D_dev : c->outD.as<float>(), I_dev, S64_dev, c->cert.as<int>(), id_offset};
    search_all(ix, c, q_dev, nq, k, Kp, out, st, kOptimisticSeedRank, true);
    if (async) return;
    c->hout.ensure((size_t)nq * sizeof(int));
    int* cert_h = (int*)c->hout.p;
    HIP_CHECK(hipMemcpyAsync(cert_h, c->cert.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // (every block's full scan has run behind its fallback round: a query left uncertified here
    // would be a library error, so it is answered by a full scan of its own rather than trusted)
    for (int64_t qi = 0; qi < nq; ++qi) {
        if (cert_h[qi]) continue;
        int* cq = c->cert.as<int>() + qi;
        HIP_CHECK(hipMemsetAsync(cq, 0, sizeof(int), st));
        full_scan_block(ix, c, q_dev + qi * ix->d, 1, k, out.at(qi, k), st, ScanOpts());
        HIP_CHECK(hipMemcpyAsync(&cert_h[qi], cq, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (!cert_h[qi]) throw VsError(VS_ERR_INTERNAL, "full scan left a query uncertified");
    }
}

// S concurrent exact device searches over consecutive parts (whole query blocks) of one batch, each
// on its own stream with its own leased workspace (leases held together, so no two parts share a
// workspace and serialise on it); a part's full-scanned queries count in unres[part] (if given).  The IVF
// coarse assignment: one 256-row block of a small quantizer fills only nlist / 256 workgroups.
void vs::search_exact_device_parts(vs_index* ix, const float* q_dev, int64_t nq, int k, int64_t* I_dev,
                                   hipStream_t* streams, int S, unsigned* unres, float* D_dev, double* S64_dev) {
    check_index(ix);
    if (nq <= 0) return;
    std::shared_lock<std::shared_mutex> lk(ix->rw);
    DeviceGuard dg(ix->device);
    if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
    std::vector<std::unique_ptr<CtxLease>> leases;
    for (int i = 0; i < S; ++i) leases.emplace_back(new CtxLease(ix, streams[i], false));
    const int Kp = screen_depth(k);
    const int64_t blocks = (nq + MFMA_QB - 1) / MFMA_QB;
    for (int i = 0; i < S; ++i) {
        const int64_t q0 = std::min(nq, blocks * i / S * MFMA_QB), q1 = std::min(nq, blocks * (i + 1) / S * MFMA_QB);
        if (q1 <= q0) continue;
        Ctx* c = leases[i]->c;
        if (!D_dev) c->outD.ensure((size_t)(q1 - q0) * k * sizeof(float));
        c->cert.ensure((size_t)(q1 - q0) * sizeof(int));
        UnresScope us(c, unres ? unres + i : nullptr);  // reset even if search_all throws
        const SearchOut out{D_dev ? D_dev + q0 * k : c->outD.as<float>(), I_dev + q0 * k,
                            S64_dev ? S64_dev + q0 * k : nullptr, c->cert.as<int>()};
        search_all(ix, c, q_dev + q0 * ix->d, q1 - q0, k, Kp, out, streams[i], kOptimisticSeedRank, true);
    }
}

// ---- two-phase exact device search (the sharded step with a global T' exchange) ----
// Phase A of every shard scores the best KA keys of each query's survivor list; the shards exchange
// those top-k lists, and the merged k-th best (a lower bound of the global k-th best score) is the
// floor under which phase B scores nothing and the certificate needs nothing: each shard then
// scores about its share of the global refine window instead of a whole window of its own.
// Applies to one int8 MFMA block of a bf16/f16 index (static: the same answer on every rank of a
// collective); otherwise phase A runs the whole exact search and phase B returns its result.
struct vs_pending {
    vs_index* ix = nullptr;
    std::shared_lock<std::shared_mutex> lk;
    std::unique_ptr<CtxLease> L;
    hipStream_t st = nullptr;
    const float* q = nullptr;
    int64_t nq = 0;
    int k = 0, ka = 0, stride = 1;
    int64_t id_offset = 0;
    bool two = false;
    RefineArgs r{};
};

bool vs::two_phase_ok(const vs_index* ix, int64_t nq, int k) {
    return ix->screen == VS_SCREEN_I8 && nq > GEMV_NQ_MAX && nq <= MFMA_QB && k <= I8_MAX_K;
}

vs_pending* vs::search_phase_a(vs_index* ix, const float* q_dev, int64_t nq, int k, int world, int64_t id_offset,
                               double* S_a, int64_t* I_a, int stride, hipStream_t st) {
    check_index(ix);
    if (k <= 0 || nq <= 0 || world <= 0) throw VsError(VS_ERR_ARG, "nq, k and world must be > 0");
    if (stride < 1) throw VsError(VS_ERR_ARG, "stride must be >= 1");
    if (ix->ntotal == 0) throw VsError(VS_ERR_ARG, "index is empty");
    std::unique_ptr<vs_pending> p(new vs_pending());
    p->ix = ix;
    p->lk = std::shared_lock<std::shared_mutex>(ix->rw);
    DeviceGuard dg(ix->device);
    p->L.reset(new CtxLease(ix, st, false));
    Ctx* c = p->L->c;
    p->st = st;
    p->q = q_dev;
    p->nq = nq;
    p->k = k;
    p->id_offset = id_offset;
    if (!two_phase_ok(ix, nq, k)) throw VsError(VS_ERR_ARG, "two-phase search: not applicable (vs_two_phase_ok)");
    // (routed to the native screen, or group-residual codes on a shard too small for their seeded
    // direct pass: phase A runs the whole search -- a per-rank choice, the exchanges are the same)
    p->two = i8_allowed(ix) && use_i8(ix, (int)nq, k);
    c->cert.ensure((size_t)nq * sizeof(int));
    if (p->two) {
        // phase A's depth: twice a shard's expected share of the global top-k (+24), so the shards'
        // lists together hold the global k-th best of what they scored
        const int share = (k + world - 1) / world;
        p->ka = (int)std::min<int64_t>(round_up(2 * k + 24, 8), round_up(2 * share + 24, 8));
        // the seed's union covers this shard's share of the global window: phase B certifies the
        // unlisted rows against the global floor (~ the global k-th best), and the shard's rows
        // within the int8 error budget of it are ~1/world of the whole window (iid shards)
        I8Opts o;
        o.phase = 1;
        o.ka = p->ka;
        o.keep = &p->r;
        o.kwin = share;
        o.prepack = true;
        search_block_i8(ix, c, q_dev, (int)nq, k, SearchOut{nullptr, I_a, S_a, c->cert.as<int>(), id_offset, stride}, st, o);
    } else {
        c->outS.ensure((size_t)nq * k * sizeof(double));
        c->outI.ensure((size_t)nq * k * sizeof(int64_t));
        c->outD.ensure((size_t)nq * k * sizeof(float));
        const SearchOut out{c->outD.as<float>(), c->outI.as<int64_t>(), c->outS.as<double>(), c->cert.as<int>(), id_offset};
        search_all(ix, c, q_dev, nq, k, screen_depth(k), out, st, kOptimisticSeedRank, true);
        HIP_CHECK(hipMemcpy2DAsync(S_a, (size_t)stride * 8, c->outS.p, 8, 8, (size_t)nq * k, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemcpy2DAsync(I_a, (size_t)stride * 8, c->outI.p, 8, 8, (size_t)nq * k, hipMemcpyDeviceToDevice, st));
    }
    return p.release();
}

void vs::search_phase_b(vs_pending* p, const double* floor_S, float* D, int64_t* I, double* S64, int stride,
                        hipStream_t st, unsigned* unres) {
    std::unique_ptr<vs_pending> own(p);
    vs_index* ix = p->ix;
    DeviceGuard dg(ix->device);
    Ctx* c = p->L->c;
    if (st != p->st) {  // order the caller's stream behind phase A's work
        DevEvent e(hipEventDisableTiming);
        HIP_CHECK(hipEventRecord(e, p->st));
        HIP_CHECK(hipStreamWaitEvent(st, e, 0));
        p->L->st = st;
    }
    const int64_t nq = p->nq;
    const int k = p->k;
    if (stride < 1) throw VsError(VS_ERR_ARG, "stride must be >= 1");
    if (!p->two) {
        HIP_CHECK(hipMemcpy2DAsync(I, (size_t)stride * 8, c->outI.p, 8, 8, (size_t)nq * k, hipMemcpyDeviceToDevice, st));
        if (S64)
            HIP_CHECK(hipMemcpy2DAsync(S64, (size_t)stride * 8, c->outS.p, 8, 8, (size_t)nq * k, hipMemcpyDeviceToDevice, st));
        if (D) HIP_CHECK(hipMemcpyAsync(D, c->outD.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToDevice, st));
        return;
    }
    RefineArgs r = p->r;
    r.phase = 2;
    r.tfloor = floor_S;
    r.tfloor_k = k;
    r.D = D;
    r.I = I;
    r.S64 = S64;
    r.ostride = stride;
    HIP_CHECK(launch_refine_wide(r, (int)nq, p->ka, st));
    health_note(ix, c, st, 1, (int)nq);
    // the block's gated fallback round (native screen, local certificate), as search_all's
    UnresScope us(c, unres);
    const SearchOut out{D, I, S64, c->cert.as<int>(), p->id_offset, stride};
    BlockOpts redo;
    redo.redo = true;
    search_block(ix, c, p->q, (int)nq, k, std::max(screen_depth(k), fallback_depth(ix)), out, st, redo);
    // and its gated full scan (the shard's own exact top-k; the floor is not needed for it)
    ScanOpts scan;
    scan.gate = c->fails.as<int>() + 1;
    full_scan_block(ix, c, p->q, (int)nq, k, out, st, scan);
}

void vs::search_pending_free(vs_pending* p) { delete p; }

namespace vs {

void check_k(int k, int kmax) {
    if (k > kmax) throw VsError(VS_ERR_ARG, "k too large (max " + std::to_string(K_MAX) + ")");
}

// The caller's buffers are pageable: a huge batch never pins its whole size for the index's life.
int64_t stage_chunk(const vs_index* ix, int64_t nq, int kk, bool with_cert) {
    const size_t per_q = std::max((size_t)ix->d * sizeof(float),
                                  (size_t)kk * (sizeof(int64_t) + sizeof(float)) + (with_cert ? sizeof(int) : 0));
    int64_t chunk = std::max<int64_t>(1, (int64_t)(kPinnedStageCap / per_q));
    if (chunk >= MFMA_QB) chunk = chunk / MFMA_QB * MFMA_QB;
    return std::min(chunk, nq);
}

// queries [q0, q0 + m) of the caller's batch -> c->qdev, through c->hq (the first chunk of a call is
// its largest; the stream was waited for since the last copy from hq)
void stage_queries(const vs_index* ix, Ctx* c, const float* q, int64_t q0, int64_t m, hipStream_t st) {
    const size_t bytes = (size_t)m * ix->d * sizeof(float);
    c->qdev.ensure(bytes);
    c->hq.ensure(bytes);
    std::memcpy(c->hq.p, q + q0 * ix->d, bytes);
    HIP_CHECK(hipMemcpyAsync(c->qdev.p, c->hq.p, bytes, hipMemcpyHostToDevice, st));
}

static StagedOut staged_out(Ctx* c, int64_t m, int kk, bool with_cert) {
    StagedOut o{};
    o.bytes = (size_t)m * kk * (sizeof(int64_t) + sizeof(float)) + (with_cert ? (size_t)m * sizeof(int) : 0);
    c->hout.ensure(o.bytes);
    c->outAll.ensure(o.bytes);
    o.Ik = (int64_t*)c->hout.p;
    o.Dk = (float*)(o.Ik + (size_t)m * kk);
    o.Id = c->outAll.as<int64_t>();
    o.Dd = (float*)(o.Id + (size_t)m * kk);
    if (with_cert) {
        o.cert_h = (int*)(o.Dk + (size_t)m * kk);
        o.cert_d = (int*)(o.Dd + (size_t)m * kk);
    }
    return o;
}

static void fetch_staged(Ctx* c, const StagedOut& o, hipStream_t st) {
    HIP_CHECK(hipMemcpyAsync(c->hout.p, c->outAll.p, o.bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

float worst_score(const vs_index* ix) { return ix->metric == VS_METRIC_IP ? -3.402823466e+38f : 3.402823466e+38f; }

void fill_padding(float* D, int64_t* I, int64_t n, float fillD) {
    for (int64_t i = 0; i < n; ++i) {
        D[i] = fillD;
        I[i] = -1;
    }
}

void scatter_padded(const StagedOut& o, int64_t q0, int64_t m, int k, int kk, float fillD, float* D, int64_t* I) {
    for (int64_t qi = 0; qi < m; ++qi) {
        float* Dq = D + (q0 + qi) * k;
        int64_t* Iq = I + (q0 + qi) * k;
        std::copy(o.Dk + qi * kk, o.Dk + (qi + 1) * kk, Dq);
        std::copy(o.Ik + qi * kk, o.Ik + (qi + 1) * kk, Iq);
        fill_padding(Dq + kk, Iq + kk, k - kk, fillD);
    }
}

// vs_search's road from a staged chunk on: the m queries in c->qdev searched at depth kk into so's
// device block, fetched to its host block, certificate failures re-searched one by one (4x deeper
// screens, then the exact full scan) into the host block -- and, with mirror, into the device block
// too (a kernel reads the lists afterwards).  Synchronises st.
static void search_staged(vs_index* ix, Ctx* c, int64_t m, int kk, const StagedOut& so, hipStream_t st, bool mirror) {
    c->outD.ensure((size_t)kk * sizeof(float));
    c->outI.ensure((size_t)kk * sizeof(int64_t));
    c->cert.ensure(sizeof(int));
    const int Kp = screen_depth(kk);
    const SearchOut one{c->outD.as<float>(), c->outI.as<int64_t>(), nullptr, c->cert.as<int>()};  // a re-searched query
    search_all(ix, c, c->qdev.as<float>(), m, kk, Kp, SearchOut{so.Dd, so.Id, nullptr, so.cert_d}, st, kOptimisticSeedRank);
    fetch_staged(c, so, st);
    // exactness certificate failed for some queries (near-ties deeper than the margin):
    // re-screen those queries one at a time with a 4x deeper candidate set; past the
    // deepest screen (more than KP_MAX rows tied within its margin) the exact full scan
    for (int64_t qi = 0; qi < m; ++qi) {
        int Kr = Kp;
        while (!so.cert_h[qi]) {
            if (Kr < 0) throw VsError(VS_ERR_INTERNAL, "full scan left a query uncertified");
            if (Kr >= KP_MAX || Kr >= ix->ntotal) {
                HIP_CHECK(hipMemsetAsync(c->cert.p, 0, sizeof(int), st));
                full_scan_block(ix, c, c->qdev.as<float>() + qi * ix->d, 1, kk, one, st, ScanOpts());
                Kr = -1;
            } else {
                Kr = (int)std::min<int64_t>(std::min<int64_t>((int64_t)Kr * 4, KP_MAX), round_up(ix->ntotal, 16));
                search_all(ix, c, c->qdev.as<float>() + qi * ix->d, 1, kk, Kr, one, st, /*safe seed*/ 0);
            }
            HIP_CHECK(hipMemcpyAsync(so.Dk + qi * kk, c->outD.p, kk * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(so.Ik + qi * kk, c->outI.p, kk * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(&so.cert_h[qi], c->cert.p, sizeof(int), hipMemcpyDeviceToHost, st));
            if (mirror) {
                HIP_CHECK(hipMemcpyAsync(so.Dd + qi * kk, c->outD.p, kk * sizeof(float), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipMemcpyAsync(so.Id + qi * kk, c->outI.p, kk * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
            }
            HIP_CHECK(hipStreamSynchronize(st));
        }
    }
}

StagedOut exact_lists(vs_index* ix, Ctx* c, const vs_sel* sel, const SelPlan& plan, int64_t m, int kk, unsigned want,
                      hipStream_t st) {
    StagedOut so = staged_out(c, m, kk, !sel);
    if (!sel) {  // (the host block is fetched either way: the certificates are read there)
        search_staged(ix, c, m, kk, so, st, (want & LISTS_DEVICE) != 0);
        return so;
    }
    so.redo = sel_search_ctx(ix, c, sel, plan, c->qdev.as<float>(), m, kk, SearchOut{so.Dd, so.Id}, st);
    if (want & LISTS_HOST) fetch_staged(c, so, st);
    return so;
}

}  // namespace vs

extern "C" {

int vs_search_device(vs_index* ix, const float* q_dev, int64_t nq, int32_t k, float* D_dev, int64_t* I_dev,
                     double* S64_dev, int64_t id_offset, void* stream) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
        check_k(k, KP_MAX);
        if (nq == 0) return;
        if (!q_dev || !I_dev) throw VsError(VS_ERR_ARG, "null device buffer");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        // NULL is the legacy default stream (torch's default stream handle is 0), never the
        // index's private non-blocking stream: that one is unordered with the caller's producers
        hipStream_t st = (hipStream_t)stream;
        if (ix->ntotal == 0) throw VsError(VS_ERR_ARG, "index is empty");
        CtxLease L(ix, st, false);
        search_all(ix, L.c, q_dev, nq, k, screen_depth(k), SearchOut{D_dev, I_dev, S64_dev, nullptr, id_offset}, st,
                   kOptimisticSeedRank);
    });
}

int vs_search_device_exact(vs_index* ix, const float* q_dev, int64_t nq, int32_t k, float* D_dev, int64_t* I_dev,
                           double* S64_dev, int64_t id_offset, void* stream) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
        check_k(k, KP_MAX);
        if (nq == 0) return;
        if (!q_dev || !I_dev) throw VsError(VS_ERR_ARG, "null device buffer");
        if (ix->ntotal == 0) throw VsError(VS_ERR_ARG, "index is empty");
        search_exact_device(ix, q_dev, nq, k, I_dev, S64_dev, (hipStream_t)stream, D_dev, id_offset, /*async*/ true);
    });
}

int vs_two_phase_ok(vs_index* ix, int64_t nq, int32_t k) {
    if (!ix) return VS_ERR_ARG;
    return two_phase_ok(ix, nq, k) ? 1 : 0;
}

int vs_search_device_phase_a(vs_index* ix, const float* q_dev, int64_t nq, int32_t k, int32_t world,
                             int64_t id_offset, double* S_a, int64_t* I_a, int32_t stride, void* stream,
                             vs_pending** out) {
    return guarded([&] {
        if (!out || !q_dev || !S_a || !I_a) throw VsError(VS_ERR_ARG, "null argument");
        *out = nullptr;
        check_k(k, KP_MAX);
        *out = search_phase_a(ix, q_dev, nq, k, world, id_offset, S_a, I_a, stride, (hipStream_t)stream);
    });
}

int vs_search_device_phase_b(vs_pending* p, const double* floor_S, float* D_dev, int64_t* I_dev, double* S64_dev,
                             int32_t stride, void* stream) {
    return guarded([&] {
        if (!p) throw VsError(VS_ERR_ARG, "null pending search");
        if (!floor_S || !I_dev) {
            search_pending_free(p);
            throw VsError(VS_ERR_ARG, "null device buffer");
        }
        search_phase_b(p, floor_S, D_dev, I_dev, S64_dev, stride, (hipStream_t)stream);
    });
}

void vs_search_pending_free(vs_pending* p) { search_pending_free(p); }

int vs_search(vs_index* ix, const float* q, int64_t nq, int32_t k, float* D, int64_t* I) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
        if (nq == 0) return;
        if (!q || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        const float fillD = worst_score(ix);
        if (ix->ntotal == 0) {
            fill_padding(D, I, nq * k, fillD);
            return;
        }
        // k beyond the rows present: search min(k, ntotal), pad the rest (faiss layout)
        const int kk = (int)std::min<int64_t>(k, ix->ntotal);
        check_k(kk);
        CtxLease L(ix, nullptr, true);
        Ctx* c = L.c;
        hipStream_t st = c->stream;
        const int64_t chunk = stage_chunk(ix, nq, kk, true);
        for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
            const int64_t m = std::min(chunk, nq - q0);
            stage_queries(ix, c, q, q0, m, st);
            const StagedOut so = exact_lists(ix, c, nullptr, SelPlan{0, 0}, m, kk, LISTS_HOST, st);
            scatter_padded(so, q0, m, k, kk, fillD, D, I);
        }
    });
}

}  // extern "C"

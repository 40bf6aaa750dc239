// vs_dbscan_host.hip -- host side of the density clusters (include/vs.h "density clusters"; kernels:
// vs_dbscan.hip over vs_range_scan.h).
//
// db_pass is the self-join of the duplicate groups (vs_components_host.hip: members ascending, VS_SELF_ABOVE,
// blocks of MFMA_QB gathered on the device, the row0 rule or the selector-tail rule) with a sink and a mask of
// the queries to answer, through the range search's tiers (range_tiers, vs_range_tiers.h).  vs_range_degrees
// is pass 1 (degree sink, every query) and a readback; vs_range_dbscan is pass 1, k_db_core, pass 2 (cluster
// sink, the queries that met an edge in pass 1) and the labels.
#include "vs_range_tiers.h"

using namespace vs;

namespace {

struct DbStats {
    int64_t members = 0, edges = 0, clusters = 0, core = 0, border = 0, noise = 0, tier = VS_RANGE_SCAN;
    int64_t rescanned[2] = {0, 0}, blocks[2] = {0, 0}, skipped = 0;
    double ms[5] = {0, 0, 0, 0, 0};
};

void db_note(vs_index* ix, const DbStats& s) {
    std::lock_guard<std::mutex> g(ix->db_mu);
    const int64_t st[12] = {s.members, s.edges,        s.clusters,  s.core,         s.border,    s.noise,
                            s.tier,    s.rescanned[0], s.blocks[0], s.rescanned[1], s.blocks[1], s.skipped};
    std::copy(st, st + 12, ix->db_stats);
    std::copy(s.ms, s.ms + 5, ix->db_times);
}

// the state of one call: the members, the block counters and the staging shared by both passes
struct DbCall {
    vs_index* ix;
    const vs_sel* sel;
    Ctx* c;
    hipStream_t st;
    int64_t n, m, nblocks;
    int mode;
    const int64_t* mem;       // [m] the members' ids, ascending (device)
    unsigned long long* cnt;  // [nblocks][MFMA_QB] pass 1's edges above each query (device)
    RangeAuxHead h;           // (the radii are uploaded once per call)
};

// One pass of the self-join.  active: per member position, whether the query is to be answered (null: all);
// a block without an active query is not staged at all.  pass: 0 or 1, the slot of the stats and times.
void db_pass(DbCall& k, const DbSinkArgs& sink, const unsigned long long* active, int pass, DbStats& stt) {
    vs_index* ix = k.ix;
    Ctx* c = k.c;
    hipStream_t st = k.st;
    DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
    int64_t block = 0;
    for (int64_t q0 = 0; q0 < k.m; q0 += MFMA_QB, ++block) {
        const int nqb = (int)std::min<int64_t>(MFMA_QB, k.m - q0);
        if (active && std::all_of(active + q0, active + q0 + nqb, [](unsigned long long v) { return v == 0ull; }))
            continue;  // (no gather, no screen, no scan)
        ++stt.blocks[pass];
        HIP_CHECK(hipEventRecord(e0, st));
        HIP_CHECK(launch_gather_rows(ix->dtype, ix->data, k.mem + q0, nqb, ix->d, ix->dpad, c->qdev.as<float>(), st));
        RangeArgs a = range_index_args(ix);
        a.n_valid = k.n;
        a.q = c->qdev.as<float>();
        a.nq = nqb;
        a.radius = range_aux_radius(c);
        a.cnt = k.cnt + block * MFMA_QB;
        a.self = k.mem + q0;
        a.self_mode = VS_SELF_ABOVE;
        // without a selector the members are the rows themselves: the block's smallest id is q0, and no
        // row below it passes for any of its queries
        a.row0 = k.sel ? 0 : q0;
        // with a selector the scan's sequence is the tail of its ascending list from the block's own first
        // position: the entries before it are below every self id of the block
        // (k.h outlives the copy from it: the block ends with a stream synchronisation)
        const RangeTiers t = range_tiers(
            ix, c, a, k.h, nqb, k.sel ? k.sel->ids + q0 : nullptr, k.sel ? k.m - q0 : 0, k.sel ? k.m - q0 : k.n - q0,
            active ? active + q0 : nullptr, k.sel, k.mode, st, e1,
            [&](const RangeArgs& r, const ScreenArgs& s, int ny) {
                HIP_CHECK(launch_db_refine(r, sink, s.glist, s.gcnt, s.lcap, ny, st));
            },
            [&](const RangeArgs& r, int G, int qy, const uint32_t* ids, int64_t mseq) {
                HIP_CHECK(launch_db_scan(r, sink, G, qy, ids, mseq, st));
            });
        if (t.screened) stt.tier = VS_RANGE_SCREEN;
        stt.rescanned[pass] += t.rescanned;
        HIP_CHECK(hipEventRecord(e2, st));
        HIP_CHECK(hipStreamSynchronize(st));
        stt.ms[2 * pass] += ms_between(e0, e1);
        stt.ms[2 * pass + 1] += ms_between(e1, e2);
    }
}

// Both entry points.  labels null: the neighbour counts alone (degrees required).
void db_run(vs_index* ix, const vs_sel* sel, float radius, int64_t min_samples, int64_t* labels, uint8_t* kinds,
            int64_t* degrees, int64_t* counts, int64_t* n_edges, bool clusters) {
    check_index(ix);
    if (std::isnan(radius)) throw VsError(VS_ERR_ARG, "radius is NaN");
    if (clusters && min_samples < 1) throw VsError(VS_ERR_ARG, "min_samples must be >= 1");
    std::shared_lock<std::shared_mutex> lk(ix->rw);
    if (sel) check_sel(ix, sel);
    const int64_t n = ix->ntotal;
    if (n > 0 && clusters && !labels) throw VsError(VS_ERR_ARG, "labels is null");
    if (n > 0 && !clusters && !degrees) throw VsError(VS_ERR_ARG, "degrees is null");
    if (counts) std::fill(counts, counts + 4, (int64_t)0);
    if (n_edges) *n_edges = 0;
    DbStats stt;
    const int64_t m = sel ? sel->m : n;  // (a selector covers rows below n only: check_sel)
    if (m == 0) {                        // an empty index, or nothing allowed: no members
        if (labels) std::fill(labels, labels + n, (int64_t)-1);
        if (kinds) std::fill(kinds, kinds + n, (uint8_t)VS_DBSCAN_NONE);
        if (degrees) std::fill(degrees, degrees + n, (int64_t)-1);
        db_note(ix, stt);
        return;
    }
    stt.members = m;
    DeviceGuard dg(ix->device);
    CtxLease L(ix, nullptr, true);
    DbCall k{};
    k.ix = ix;
    k.sel = sel;
    k.c = L.c;
    k.st = L.c->stream;
    k.n = n;
    k.m = m;
    k.nblocks = (m + MFMA_QB - 1) / MFMA_QB;
    k.mode = ix->range_mode.load();
    Ctx* c = k.c;
    hipStream_t st = k.st;
    const uint32_t* sel_ids = sel ? sel->ids : nullptr;
    // (counted in vs_device_bytes_live, freed when the call returns)
    DevBuf deg, cnt, parent, core, best, labels_d, kinds_d, degrees_d;
    const size_t cnt_bytes = (size_t)k.nblocks * MFMA_QB * sizeof(unsigned long long);
    deg.ensure((size_t)n * sizeof(uint32_t));
    cnt.ensure(cnt_bytes);
    degrees_d.ensure((size_t)n * sizeof(int64_t));
    HIP_CHECK(hipMemsetAsync(deg.p, 0, (size_t)n * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, cnt_bytes, st));
    k.cnt = cnt.as<unsigned long long>();
    // the members' ids, ascending: the queries' rows and their self ids
    c->row_ids.ensure((size_t)m * sizeof(int64_t));
    HIP_CHECK(launch_km_members(sel_ids, m, c->row_ids.as<int64_t>(), st));
    k.mem = c->row_ids.as<int64_t>();
    c->qdev.ensure((size_t)std::min<int64_t>(m, MFMA_QB) * ix->d * sizeof(float));
    c->rng_aux.ensure(sizeof(RangeAuxHead));
    std::fill(k.h.radius, k.h.radius + MFMA_QB, radius);
    HIP_CHECK(hipMemcpyAsync(c->rng_aux.p, k.h.radius, sizeof(k.h.radius), hipMemcpyHostToDevice, st));

    // pass 1: the degrees, and each query's edges above
    DbSinkArgs s1{};
    s1.deg = deg.as<uint32_t>();
    db_pass(k, s1, nullptr, 0, stt);
    std::vector<unsigned long long> cnt_h((size_t)k.nblocks * MFMA_QB);
    HIP_CHECK(hipMemcpyAsync(cnt_h.data(), cnt.p, cnt_bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < m; ++i) stt.edges += (int64_t)cnt_h[(size_t)i];

    DbLabelArgs la{};
    la.deg = deg.as<uint32_t>();
    la.sel_ids = sel_ids;
    la.m = m;
    la.n = n;
    la.degrees = degrees_d.as<int64_t>();
    if (clusters) {
        parent.ensure((size_t)n * sizeof(uint32_t));
        core.ensure((size_t)n);
        best.ensure((size_t)n * sizeof(unsigned long long));
        labels_d.ensure((size_t)n * sizeof(int64_t));
        kinds_d.ensure((size_t)n);
        HIP_CHECK(launch_cc_init(parent.as<uint32_t>(), n, st));
        HIP_CHECK(hipMemsetAsync(core.p, 0, (size_t)n, st));
        HIP_CHECK(hipMemsetAsync(best.p, 0, (size_t)n * sizeof(unsigned long long), st));
        HIP_CHECK(launch_db_core(deg.as<uint32_t>(), sel_ids, m, n, min_samples, core.as<uint8_t>(), st));
        // pass 2: a query that met no edge above meets none now
        for (int64_t i = 0; i < m; ++i) stt.skipped += cnt_h[(size_t)i] == 0ull ? 1 : 0;
        DbSinkArgs s2{};
        s2.parent = parent.as<uint32_t>();
        s2.core = core.as<uint8_t>();
        s2.best = best.as<unsigned long long>();
        db_pass(k, s2, cnt_h.data(), 1, stt);
        la.parent = parent.as<uint32_t>();
        la.core = core.as<uint8_t>();
        la.best = best.as<unsigned long long>();
        la.labels = labels_d.as<int64_t>();
        la.kinds = kinds_d.as<uint8_t>();
    }
    // labels, kinds and degrees of every member, over a -1 / 0 / -1 fill (rows that are no members)
    DevEvent e0(hipEventDefault), e1(hipEventDefault);
    HIP_CHECK(hipEventRecord(e0, st));
    HIP_CHECK(hipMemsetAsync(degrees_d.p, 0xFF, (size_t)n * sizeof(int64_t), st));
    if (clusters) {
        HIP_CHECK(hipMemsetAsync(labels_d.p, 0xFF, (size_t)n * sizeof(int64_t), st));
        HIP_CHECK(hipMemsetAsync(kinds_d.p, 0, (size_t)n, st));
    }
    HIP_CHECK(launch_db_labels(la, st));
    std::vector<uint8_t> kinds_h;
    std::vector<int64_t> degrees_h;
    if (clusters) {
        if (!kinds) {
            kinds_h.resize((size_t)n);
            kinds = kinds_h.data();
        }
        HIP_CHECK(hipMemcpyAsync(labels, labels_d.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(kinds, kinds_d.p, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    if (degrees) HIP_CHECK(hipMemcpyAsync(degrees, degrees_d.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    stt.ms[4] = ms_between(e0, e1);
    if (clusters) {
        for (int64_t i = 0; i < n; ++i) {
            stt.core += kinds[i] == VS_DBSCAN_CORE ? 1 : 0;
            stt.border += kinds[i] == VS_DBSCAN_BORDER ? 1 : 0;
            stt.noise += kinds[i] == VS_DBSCAN_NOISE ? 1 : 0;
            stt.clusters += kinds[i] == VS_DBSCAN_CORE && labels[i] == i ? 1 : 0;
        }
        if (counts) {
            counts[0] = stt.clusters;
            counts[1] = stt.core;
            counts[2] = stt.border;
            counts[3] = stt.noise;
        }
    }
    if (n_edges) *n_edges = stt.edges;
    db_note(ix, stt);
}

}  // namespace

extern "C" {

int vs_range_degrees(vs_index* ix, const vs_sel* sel, float radius, int64_t* degrees, int64_t* n_edges) {
    return guarded([&] { db_run(ix, sel, radius, 1, nullptr, nullptr, degrees, nullptr, n_edges, false); });
}

int vs_range_dbscan(vs_index* ix, const vs_sel* sel, float radius, int64_t min_samples, int64_t* labels, uint8_t* kinds,
                    int64_t* degrees, int64_t* counts, int64_t* n_edges) {
    return guarded([&] { db_run(ix, sel, radius, min_samples, labels, kinds, degrees, counts, n_edges, true); });
}

int vs_dbscan_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->db_mu, ix->db_stats, 12, out, cap, "stats");
    });
}

int vs_dbscan_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->db_mu, ix->db_times, 5, out, cap, "times");
    });
}

}  // extern "C"

// vs_dbscan.hip -- exact density clusters: neighbour counts per row and core-point DBSCAN over the stored
// rows (include/vs.h "density clusters").
//
// The kernels are the range search's (vs_range_scan.h) with two more sinks over the self-join of the
// duplicate groups (members as queries, VS_SELF_ABOVE: every edge is met once, from its lower end):
//   * pass 1, RsDegreeSink: an edge adds 1 to either end's degree and to the query's "edges above" counter.
//   * k_db_core: core[id] = deg[id] + 1 >= min_samples over the members.
//   * pass 2, RsDbscanSink: core - core edges unite (cc_unite), core - non-core edges offer the core row to
//     the other end's best[] (a 64-bit atomicMax), the rest do nothing.
//   * k_db_labels: labels, kinds and degrees of every member, over the host's -1 / 0 / -1 fill.
// Every store is an atomic into deg / parent / best [0, n_valid) or a plain vector store into core / labels /
// kinds / degrees [0, n_valid), arrays the host sized; every id is below n_valid before it indexes any.
#include "vs_range_scan.h"

namespace vs {

constexpr int DB_THREADS = 256;

static int db_blocks(int64_t n) { return (int)((n + DB_THREADS - 1) / DB_THREADS); }

// member i of m: row sel_ids[i] (null: row i); rows at or past n are skipped (never an address outside)
__global__ void __launch_bounds__(DB_THREADS) k_db_core(const uint32_t* __restrict__ deg,
                                                        const uint32_t* __restrict__ sel_ids, int64_t m, int64_t n,
                                                        int64_t min_samples, uint8_t* __restrict__ core) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= m) return;
    const int64_t id = sel_ids ? (int64_t)sel_ids[i] : i;
    if (id >= n) return;
    core[id] = (int64_t)deg[id] + 1 >= min_samples ? 1 : 0;
}

__global__ void __launch_bounds__(DB_THREADS) k_db_labels(DbLabelArgs a) {
    const int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    if (i >= a.m) return;
    const int64_t id = a.sel_ids ? (int64_t)a.sel_ids[i] : i;
    if (id >= a.n) return;
    a.degrees[id] = (int64_t)a.deg[id];
    if (!a.labels) return;  // (the neighbour counts alone)
    int64_t label = -1;
    uint8_t kind = VS_DBSCAN_NOISE;
    const unsigned long long b = a.best[id];
    if (a.core[id]) {
        label = (int64_t)cc_find<false>(a.parent, (uint32_t)id);
        kind = VS_DBSCAN_CORE;
    } else if (b != 0ull) {
        const uint32_t cid = db_key_id(b);
        if ((int64_t)cid < a.n) {  // (a key holds a core row's id; bounded all the same)
            label = (int64_t)cc_find<false>(a.parent, cid);
            kind = VS_DBSCAN_BORDER;
        }
    }
    a.labels[id] = label;
    a.kinds[id] = kind;
}

hipError_t launch_db_core(const uint32_t* deg, const uint32_t* sel_ids, int64_t m, int64_t n, int64_t min_samples,
                          uint8_t* core, hipStream_t st) {
    if (!deg || !core || m <= 0 || n <= 0 || m > n || min_samples < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_db_core, dim3(db_blocks(m)), dim3(DB_THREADS), 0, st, deg, sel_ids, m, n, min_samples, core);
    return hipGetLastError();
}

hipError_t launch_db_labels(const DbLabelArgs& a, hipStream_t st) {
    if (!a.deg || !a.degrees || a.m <= 0 || a.n <= 0 || a.m > a.n) return hipErrorInvalidValue;
    if (a.labels && (!a.kinds || !a.parent || !a.core || !a.best)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_db_labels, dim3(db_blocks(a.m)), dim3(DB_THREADS), 0, st, a);
    return hipGetLastError();
}

// the range kernels with the degree sink (s.deg set) or the cluster sink
static bool db_args_ok(const RangeArgs& a, const DbSinkArgs& s) {
    return a.cnt && a.self && a.nq <= MFMA_QB && a.n_valid <= (int64_t)0xFFFFFFFFll && a.self_mode == VS_SELF_ABOVE &&
           (s.deg ? !s.parent : (s.parent && s.core && s.best));
}

hipError_t launch_db_scan(const RangeArgs& a, const DbSinkArgs& s, int G, int qy, const uint32_t* ids, int64_t m,
                          hipStream_t st) {
    if (!db_args_ok(a, s)) return hipErrorInvalidValue;
    if (s.deg) return rs_launch_scan<RsDegreeSink, true>(a, {s.deg}, 0, 0, G, qy, ids, m, st);
    return rs_launch_scan<RsDbscanSink, true>(a, {s.parent, s.core, s.best}, 0, 0, G, qy, ids, m, st);
}

hipError_t launch_db_refine(const RangeArgs& a, const DbSinkArgs& s, const u64* glist, const int* gcnt, int lcap, int ny,
                            hipStream_t st) {
    if (!db_args_ok(a, s)) return hipErrorInvalidValue;
    if (s.deg) return rs_launch_refine<RsDegreeSink, true>(a, {s.deg}, glist, gcnt, lcap, ny, st);
    return rs_launch_refine<RsDbscanSink, true>(a, {s.parent, s.core, s.best}, glist, gcnt, lcap, ny, st);
}

}  // namespace vs

// vs_components.hip -- exact duplicate groups: the connected components of the "within a radius" relation
// over the stored rows (include/vs.h "duplicate groups").
//
// The kernels are the range search's (vs_range_scan.h) with a third sink: the members are the queries
// (gathered from their own rows, VS_SELF_ABOVE, so every edge is met once, from its lower end), the scan's
// K loop, its exact_score_rows call and its predicate are the same code, and a row that passes is united
// with the query's row in a lock-free union-find instead of being appended to a pair buffer.
//   * k_cc_init: parent[i] = i.
//   * k_range_scan with the union sink (SCAN tier) / k_range_refine with it (SCREEN tier): lane 0 of a wave
//     holds its R rows' scores, adds the passing ones to the query's edge counter with one atomic and unites
//     each with the query's row (cc_unite, vs_range_scan.h: the larger root is hooked under the smaller by a
//     CAS, so a tree's root is its smallest id and the result does not depend on the order of the unions).
//   * k_cc_labels: labels[id] = find(id) for every member, over a -1 fill.
// Every store is an atomic into parent[0, n_valid) or a plain vector store into labels[0, n_valid), arrays
// the host sized; every id is below n_valid before it indexes either.
#include "vs_range_scan.h"

namespace vs {

constexpr int CC_THREADS = 256;

__global__ void __launch_bounds__(CC_THREADS) k_cc_init(uint32_t* __restrict__ parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

// member i of m: row sel_ids[i] (null: row i); rows at or past n are skipped (never an address outside)
__global__ void __launch_bounds__(CC_THREADS) k_cc_labels(uint32_t* __restrict__ parent,
                                                          const uint32_t* __restrict__ sel_ids, int64_t m, int64_t n,
                                                          int64_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= m) return;
    const int64_t id = sel_ids ? (int64_t)sel_ids[i] : i;
    if (id >= n) return;
    labels[id] = (int64_t)cc_find<false>(parent, (uint32_t)id);
}

static int cc_blocks(int64_t n) { return (int)((n + CC_THREADS - 1) / CC_THREADS); }

hipError_t launch_cc_init(uint32_t* parent, int64_t n, hipStream_t st) {
    if (!parent || n <= 0 || n > (int64_t)0xFFFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cc_init, dim3(cc_blocks(n)), dim3(CC_THREADS), 0, st, parent, n);
    return hipGetLastError();
}

hipError_t launch_cc_labels(uint32_t* parent, const uint32_t* sel_ids, int64_t m, int64_t n, int64_t* labels,
                            hipStream_t st) {
    if (!parent || !labels || m <= 0 || n <= 0 || m > n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cc_labels, dim3(cc_blocks(m)), dim3(CC_THREADS), 0, st, parent, sel_ids, m, n, labels);
    return hipGetLastError();
}

// the range kernels with the union sink
static bool cc_args_ok(const RangeArgs& a, const uint32_t* parent) {
    return a.cnt && a.self && parent && a.n_valid <= (int64_t)0xFFFFFFFFll && a.self_mode == VS_SELF_ABOVE;
}

hipError_t launch_cc_scan(const RangeArgs& a, uint32_t* parent, int G, int qy, const uint32_t* ids, int64_t m,
                          hipStream_t st) {
    if (!cc_args_ok(a, parent)) return hipErrorInvalidValue;
    return rs_launch_scan<RsUnionSink, true>(a, {parent}, 0, 0, G, qy, ids, m, st);
}

hipError_t launch_cc_refine(const RangeArgs& a, uint32_t* parent, const u64* glist, const int* gcnt, int lcap, int ny,
                            hipStream_t st) {
    if (!cc_args_ok(a, parent)) return hipErrorInvalidValue;
    return rs_launch_refine<RsUnionSink, true>(a, {parent}, glist, gcnt, lcap, ny, st);
}

}  // namespace vs

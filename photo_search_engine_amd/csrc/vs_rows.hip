// vs_rows.hip -- queries taken from stored rows (include/vs.h "queries taken from stored rows"; host:
// vs_rows_host.hip).
//
// The queries of vs_search_rows / vs_range_search_rows are rows the index holds: k_gather_rows
// (vs_kernels.hip) writes them as fp32 into the context's query buffer, so no query crosses PCIe, and
// the searches that follow are the ones vs_search / vs_search_sel / vs_range_search run from their
// staged queries on.  The self-aware predicate of the range kernels lives with them (vs_range.hip,
// rs_self_ok).  What is left for this file:
//   * k_rows_take: VS_SELF_DROP of the top-k call.  The search ran at kk = min(k + 1, ntotal); one
//     wave per query finds the slot that holds the query's own row with a ballot over the list --
//     by id, not by position: an identical row with a lower id comes first -- and writes the first
//     k entries that are not that slot.  A list without the row (inner product over unnormalised
//     rows, a row the selector does not allow) keeps its first k entries.  Slots the list cannot
//     fill are padded as vs_search pads them.
// Every store is bounded by k entries of the query's own output row.  Plain vector stores only.
#include "vs_device.h"

namespace vs {

__global__ void __launch_bounds__(64) k_rows_take(RowsTakeArgs a) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t self = a.self[q];
    const int64_t* Iq = a.I_in + q * a.kk;
    // the slot holding the row itself (ids of a list are distinct: at most one), or kk = none
    int slot = a.kk;
    for (int j0 = 0; j0 < a.kk; j0 += 64) {
        const int j = j0 + lane;
        const u64 hit = __ballot(j < a.kk && Iq[j] == self);  // (wave-uniform)
        if (hit) {
            slot = j0 + __ffsll((long long)hit) - 1;
            break;
        }
    }
    for (int j = lane; j < a.k; j += 64) {
        const int src = j < slot ? j : j + 1;
        const size_t o = (size_t)q * a.k + j;
        if (src < a.kk) {
            const size_t i = (size_t)q * a.kk + src;
            a.I[o] = a.I_in[i];
            if (a.D) a.D[o] = a.D_in[i];
            if (a.S64) a.S64[o] = a.S_in[i];
        } else {
            a.I[o] = -1;
            if (a.D) a.D[o] = a.metric == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
            if (a.S64) a.S64[o] = a.metric == METRIC_L2 ? 1.7976931348623157e308 : -1.7976931348623157e308;
        }
    }
}

hipError_t launch_rows_take(const RowsTakeArgs& a, int64_t nq, hipStream_t st) {
    if (nq <= 0 || nq > 0x7FFFFFFF || a.k <= 0 || a.kk < a.k || !a.self || !a.I_in || !a.I || (a.D && !a.D_in) ||
        (a.S64 && !a.S_in) || (a.metric != METRIC_IP && a.metric != METRIC_L2))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rows_take, dim3((unsigned)nq), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace vs

// vs_fullscan.hip -- the last tier of the exactness fallback: an exact full scan of the shard.
//
// Every screen of libvs lists a bounded number of candidate rows per query (KP_MAX = 4096 in the
// deepest fallback round), and its certificate proves that no unlisted row can enter the top-k.
// When more rows than that tie (or nearly tie) at the k-th best score -- thousands of identical
// photo embeddings -- no bounded list can hold them, and faiss still answers: IndexFlatIP /
// IndexFlatL2 return the k lowest ids among equal scores (/root/reference/utils/vector_store.py:191,
// pinned by /root/reference/tests/test_searcher.py:323-350).  This kernel gives that answer for any
// number of ties: every row of the shard is scored exactly (the canonical fp64 expression tree of
// exact_score_rows, bit-identical with the oracle) and streamed through a bounded running top-k
// under the total order (score desc / distance asc, then id asc).
//
// One launch handles every query of a block whose cert[q] is 0 (optionally gated on a device count,
// so the launch returns at once when no query needs it).  Workgroup b scans the contiguous row range
// [n b / G, n (b + 1) / G): rows are scored 32 at a time (8 waves x RR rows), the ones that beat the
// workgroup's current k-th best go to an LDS batch, and a full batch is sorted (bitonic) and merged
// into the workgroup's sorted list by rank (each element's new position = its index + its rank in
// the other list).  Within a range rows come in id order, so once the list is full a row tied with
// the k-th best never enters it: the memory stays O(k) however many rows tie.  Each workgroup writes
// its list to global scratch; the last one to finish (device-scope fence + per-query counter, re-
// zeroed by it) merges the G sorted lists -- only each list's prefix that beats the running k-th
// best is read -- and writes the faiss-layout result and cert[q] = 1.
#include "vs_scan.h"

namespace vs {

// (the scan itself: fs_scan_body, vs_scan.h -- shared with the selector scan, vs_selscan.hip)
template <int DT, int METRIC, bool QLDS>
__global__ void __launch_bounds__(FS_THREADS) k_full_scan(FullScanArgs a, int KL) {
    fs_scan_body<DT, METRIC, QLDS, false>(a, KL, nullptr, 0);
}

size_t full_scan_scratch_bytes(int nq, int G, int k) { return (size_t)nq * G * k * 12; }

hipError_t launch_full_scan(const FullScanArgs& a, hipStream_t st) {
    return fs_launch_scan(a, 1, false, 1, st,
                          [](auto dt, auto metric, auto qlds, auto) { return k_full_scan<dt, metric, qlds>; });
}

}  // namespace vs

"""Fused search: FlatIndex.search_fused against what it replaces, in one process.
Corpus: the bursts of scripts/groups_timing.py (default 100k x 1536, bf16).  256 fused queries of m
sub-queries each, the "alternative wordings" unit(q[i] + spread g_j / sqrt(d)), g_j standard normal: at
the default spread of 1.27 a wording's cosine to q[i] is about 0.62 (what 0.15 noise per element gives the
d = 72 test corpus); m in 2, 4, 8 and k in 10, 100.

Per (m, k), medians over --runs after one untimed call:
  any    search_fused(mode="any") as wall time around the synchronising call, the library's HIP events
         (vs_fuse_last_times: list search and walk), and beside it the m plain FlatIndex.search calls of the
         same batch plus the host merge (union, best score per id, first k by (score, id)) as wall time.
         The merge sees fp32 scores: where two rows' fp64 scores differ but round to one fp32 value it orders
         them by id, the index by the fp64 score -- D must be equal, I may differ inside such runs
         (fp32_tie_positions counts them);
  all    search_fused(mode="all") under AUTO: wall time, HIP events per list tier, where the queries completed;
  scan   the forced SCAN tier (mode="all"): HIP-event ms of the fused scan per fused query, against m times
         the single-query exact scan of the same index -- adjusted search's SCAN tier under a plain adjustment
         (vs_adjust_last_times' full scan), per query.
One JSON line per shape, also appended to --out.
python scripts/fuse_timing.py [--out profiles/fuse_timing.jsonl] [--n 100000] [--d 1536]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from groups_timing import burst_rows  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402


def host_merge(lists, k):
    """The reference's merge of m (D, I) lists per query: the best score per id, the first k by (score, id)."""
    nq = lists[0][0].shape[0]
    D = np.full((nq, k), -np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for a in range(nq):
        best = {}
        for Dj, Ij in lists:
            for s, i in zip(Dj[a].tolist(), Ij[a].tolist()):
                if i >= 0 and (i not in best or s > best[i]):
                    best[i] = s
        page = sorted(best.items(), key=lambda t: (-t[1], t[0]))[:k]
        I[a, :len(page)] = [i for i, _ in page]
        D[a, :len(page)] = [s for _, s in page]
    return D, I


def med(v):
    return round(float(np.median(np.asarray(v, dtype=np.float64))), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ms", default="2,4,8")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--spread", type=float, default=1.27)
    args = ap.parse_args()
    n, d, nq = args.n, args.d, args.nq
    x, q, _ = burst_rows(n, d, 256, 7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 65536):
        ix.add(x[r0:r0 + 65536])
    del x
    rng = np.random.default_rng(23)
    plain_adj = ix.score_adjust(None, None)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")

    for m in [int(v) for v in args.ms.split(",")]:
        fq = q[:nq, None, :].astype(np.float64) + args.spread / np.sqrt(d) * rng.standard_normal((nq, m, d))
        fq = np.ascontiguousarray(fq / np.linalg.norm(fq, axis=2, keepdims=True), dtype=np.float32)
        subs = [np.ascontiguousarray(fq[:, j]) for j in range(m)]
        for k in [int(v) for v in args.ks.split(",")]:
            base = {"N": n, "d": d, "dtype": args.dtype, "nq": nq, "m": m, "k": k}
            # ---- ANY against m plain searches + the host merge ----
            ix.set_fuse_mode("auto")
            wall, ts, tw, plain, merge, swaps = [], [], [], [], [], 0
            for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                t0 = time.perf_counter()
                res = ix.search_fused(fq, k, "any")
                t1 = time.perf_counter()
                t = ix.fuse_last_times()
                lists = [ix.search(s, k) for s in subs]
                t2 = time.perf_counter()
                Dm, Im = host_merge(lists, k)
                t3 = time.perf_counter()
                assert np.array_equal(Dm, res[0])
                bad = Im != res[1]  # (only inside runs of equal fp32 scores)
                run_of = np.zeros_like(bad)
                run_of[:, 1:] |= Dm[:, 1:] == Dm[:, :-1]
                run_of[:, :-1] |= Dm[:, :-1] == Dm[:, 1:]
                run_of[:, -1] = True  # (the k-th row may tie with the first row left out)
                assert not (bad & ~run_of).any()
                swaps = int(bad.sum())
                if run:
                    wall.append((t1 - t0) * 1e3)
                    ts.append(t["search_ms"][0])
                    tw.append(t["walk_ms"][0])
                    plain.append((t2 - t1) * 1e3)
                    merge.append((t3 - t2) * 1e3)
            emit(dict(base, what="any", fused_wall_ms=med(wall), list_search_ms=med(ts), walk_ms=med(tw),
                      walk_over_search=round(med(tw) / med(ts), 4) if med(ts) > 0 else None,
                      m_plain_searches_wall_ms=med(plain), host_merge_wall_ms=med(merge), fp32_tie_positions=swaps))
            # ---- ALL under AUTO ----
            wall, ts, tw, tsc = [], [], [], []
            for run in range(args.runs + 1):
                t0 = time.perf_counter()
                ix.search_fused(fq, k, "all")
                t1 = time.perf_counter()
                t, st = ix.fuse_last_times(), ix.fuse_last_stats()
                if run:
                    wall.append((t1 - t0) * 1e3)
                    ts.append(t["search_ms"])
                    tw.append(t["walk_ms"])
                    tsc.append(t["scan_ms"] + t["scan_walk_ms"])
            ts, tw = np.median(np.asarray(ts), axis=0), np.median(np.asarray(tw), axis=0)
            emit(dict(base, what="all", fused_wall_ms=med(wall), search_ms_per_tier=[round(float(v), 3) for v in ts],
                      walk_ms_per_tier=[round(float(v), 3) for v in tw],
                      walk_over_search_tier1=round(float(tw[0] / ts[0]), 4) if ts[0] > 0 else None, scan_ms=med(tsc),
                      tiers=[st["first"], st["deeper"], st["scan"]], longest_list=st["longest"]))
            # ---- the SCAN tier against m single-query exact scans ----
            ix.set_fuse_mode("scan")
            ix.set_adjust_mode("scan")
            fscan, fwalk, single = [], [], []
            for run in range(args.runs + 1):
                ix.search_fused(fq, k, "all")
                t = ix.fuse_last_times()
                ix.search_adjusted(subs[0], k, plain_adj)
                ta = ix.adjust_last_times()
                if run:
                    fscan.append(t["scan_ms"])
                    fwalk.append(t["scan_walk_ms"])
                    single.append(ta["full_scan_ms"])
            ix.set_fuse_mode("auto")
            ix.set_adjust_mode("auto")
            # (both sides with the walk that reports the scan's rows: vs_adjust_last_times' full scan includes its own)
            per_fused, per_single = (med(fscan) + med(fwalk)) / nq, med(single) / nq
            emit(dict(base, what="scan", fused_scan_ms=med(fscan), fused_scan_walk_ms=med(fwalk),
                      single_scan_with_walk_ms=med(single), fused_scan_ms_per_fused_query=round(per_fused, 4),
                      m_single_scans_ms_per_fused_query=round(m * per_single, 4),
                      fused_over_m_single=round(per_fused / (m * per_single), 4) if per_single > 0 else None))
    plain_adj.close()
    ix.close()


if __name__ == "__main__":
    main()

"""Multi-vector search: FlatIndex.search_maxsim against what it replaces, in one process.
Corpus: the bursts of scripts/groups_timing.py (default 100k x 1536, bf16), grouped at random into --groups
groups (10000: about 10 rows each; 100: about 1000 each).  nq queries of m sub-queries, the "concepts"
unit(q[i + 37 j]): unrelated directions, as the concepts of one request are.

Per (groups, m, k), medians over --runs after one untimed call:
  auto   search_maxsim under AUTO: wall time around the synchronising call, HIP events per list tier
         (vs_maxsim_last_times), where the queries completed and the rows the answering walks went through;
  walk   LISTS with the row cap lifted (walk_rows = 2^40): the walk's HIP-event ms per row of the candidate
         groups, and the rows at which one query's walk would cost one query's scan -- the measurement behind
         the default walk_rows;
  scan   the forced SCAN tier: HIP-event ms of scan, rank and final walk, against the fused search forced to
         SCAN at the same m and k (vs_fuse_last_times: the same scoring loop with a running top-k in place of
         the table); at the first k also the scan's two A/Bs, through the library's measurement switch
         VS_MAXSIM_SCAN_VARIANT (1: lane 0 offers every pair instead of one lane per pair; 2: no relaxed load in
         front of the atomicMax);
  fused  --fused-only [--pkg-root DIR]: only the fused search's forced scan, with the package taken from DIR --
         a checkout of the parent commit, which has no search_maxsim -- for the same queries;
  host   the road open without the call, over --host-nq queries: m infinite-radius range_search calls, a
         NumPy group maximum, the sum and an argsort; wall time per query beside search_maxsim's.
One JSON line per shape, also appended to --out.
python scripts/maxsim_timing.py [--out profiles/maxsim_timing.jsonl] [--n 100000] [--d 1536]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if "--pkg-root" in sys.argv:  # (before the package is imported)
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--pkg-root") + 1]))
from groups_timing import burst_rows  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402


def med(v):
    return round(float(np.median(np.asarray(v, dtype=np.float64))), 3)


def host_road(ix, subs, code, ncodes, k):
    """m infinite-radius range searches, the group maximum, the sum, the first k by (F, code)."""
    nq = subs[0].shape[0]
    F = np.zeros((nq, ncodes), dtype=np.float64)
    for qj in subs:
        lims, D, I = ix.range_search(qj, -np.inf)
        for a in range(nq):
            M = np.full((ncodes,), -np.inf, dtype=np.float64)
            np.maximum.at(M, code[I[lims[a]:lims[a + 1]]], D[lims[a]:lims[a + 1]].astype(np.float64))
            F[a] += M
    return np.stack([np.lexsort((np.arange(ncodes), -F[a]))[:k] for a in range(nq)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--host-nq", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ms", default="1,4,8")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--groups", default="10000,100")
    ap.add_argument("--skip", default="", help="comma list of auto, walk, scan, host")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--pkg-root", default=None)
    args = ap.parse_args()
    n, d, nq = args.n, args.d, args.nq
    skip = set(args.skip.split(","))
    x, q, _ = burst_rows(n, d, 256, 7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 65536):
        ix.add(x[r0:r0 + 65536])
    del x
    rng = np.random.default_rng(31)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")

    if args.fused_only:
        ix.set_fuse_mode("scan")
        for m in [int(v) for v in args.ms.split(",")]:
            q3 = np.ascontiguousarray(np.stack([q[(np.arange(nq) + 37 * j) % q.shape[0]] for j in range(m)], axis=1))
            for k in [int(v) for v in args.ks.split(",")]:
                fs = []
                for run in range(args.runs + 1):
                    ix.search_fused(q3, k, "all")
                    if run:
                        fs.append(ix.fuse_last_times()["scan_ms"])
                emit({"N": n, "d": d, "dtype": args.dtype, "nq": nq, "m": m, "k": k, "what": "fused", "pkg_root": args.pkg_root,
                      "fused_scan_ms": med(fs)})
        ix.close()
        return
    ks = [int(v) for v in args.ks.split(",")]
    for ngroups in [int(v) for v in args.groups.split(",")]:
        code = rng.integers(0, ngroups, size=n).astype(np.int64)
        groups = ix.group_keys(code)
        for m in [int(v) for v in args.ms.split(",")]:
            q3 = np.ascontiguousarray(np.stack([q[(np.arange(nq) + 37 * j) % q.shape[0]] for j in range(m)], axis=1))
            for k in [int(v) for v in args.ks.split(",")]:
                base = {"N": n, "d": d, "dtype": args.dtype, "groups": ngroups, "nq": nq, "m": m, "k": k}
                auto_wall = None
                if "auto" not in skip:
                    wall, ts, tw, tsc = [], [], [], []
                    for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                        t0 = time.perf_counter()
                        ix.search_maxsim(q3, k, groups)
                        t1 = time.perf_counter()
                        t, st = ix.maxsim_last_times(), ix.maxsim_last_stats()
                        if run:
                            wall.append((t1 - t0) * 1e3)
                            ts.append(t["search_ms"])
                            tw.append(t["walk_ms"])
                            tsc.append(t["scan_ms"] + t["rank_ms"] + t["scan_walk_ms"])
                    ts, tw = np.median(np.asarray(ts), axis=0), np.median(np.asarray(tw), axis=0)
                    auto_wall = med(wall)
                    emit(dict(base, what="auto", wall_ms=auto_wall, search_ms_per_tier=[round(float(v), 3) for v in ts],
                              walk_ms_per_tier=[round(float(v), 3) for v in tw], scan_tier_ms=med(tsc),
                              tiers=[st["first"], st["deeper"], st["scan"]], longest_list=st["longest"], walked_rows=st["walked"]))
                scan_per_query = None
                if "scan" not in skip:
                    ix.set_maxsim_mode("scan")
                    ix.set_fuse_mode("scan")
                    sc, rk, wk, fs = [], [], [], []
                    try:
                        for run in range(args.runs + 1):
                            ix.search_maxsim(q3, k, groups)
                            t = ix.maxsim_last_times()
                            ix.search_fused(q3, k, "all")
                            tf = ix.fuse_last_times()
                            if run:
                                sc.append(t["scan_ms"])
                                rk.append(t["rank_ms"])
                                wk.append(t["scan_walk_ms"])
                                fs.append(tf["scan_ms"])
                    finally:
                        ix.set_maxsim_mode("auto")
                        ix.set_fuse_mode("auto")
                    scan_per_query = (med(sc) + med(rk) + med(wk)) / nq
                    ab = {}
                    if k == ks[0]:  # the scan's two A/Bs (the scan kernel alone; k does not reach it)
                        ix.set_maxsim_mode("scan")
                        try:
                            for name, variant in (("lane0_offers_all_ms", "1"), ("no_load_before_atomic_ms", "2")):
                                os.environ["VS_MAXSIM_SCAN_VARIANT"] = variant
                                v = []
                                for run in range(args.runs + 1):
                                    ix.search_maxsim(q3, k, groups)
                                    if run:
                                        v.append(ix.maxsim_last_times()["scan_ms"])
                                ab[name] = med(v)
                        finally:
                            os.environ.pop("VS_MAXSIM_SCAN_VARIANT", None)
                            ix.set_maxsim_mode("auto")
                    emit(dict(base, what="scan", **ab, scan_ms=med(sc), rank_ms=med(rk), final_walk_ms=med(wk), fused_scan_ms=med(fs),
                              scan_over_fused_scan=round(med(sc) / med(fs), 4) if med(fs) > 0 else None,
                              tier_ms_per_query=round(scan_per_query, 4)))
                if "walk" not in skip:
                    ix.set_maxsim_mode("lists")
                    ix.set_maxsim_depth(0, 0, 1 << 40)
                    ts, tw = [], []
                    try:
                        for run in range(args.runs + 1):
                            ix.search_maxsim(q3, k, groups)
                            t, st = ix.maxsim_last_times(), ix.maxsim_last_stats()
                            if run:
                                ts.append(sum(t["search_ms"]))
                                tw.append(sum(t["walk_ms"]))
                    finally:
                        ix.set_maxsim_mode("auto")
                        ix.set_maxsim_depth(0, 0, 0)
                    rows_per_query = st["walked"] / max(1, nq - st["scan"])
                    # (one workgroup walks one query: the walk's time is that of its longest query, about)
                    ms_per_row = med(tw) / max(1.0, rows_per_query) / max(1, -(-nq // 256))
                    emit(dict(base, what="walk", list_search_ms=med(ts), walk_ms=med(tw), tiers=[st["first"], st["deeper"], st["scan"]],
                              walked_rows_per_query=round(rows_per_query, 1), walk_us_per_row=round(1e3 * ms_per_row, 4),
                              rows_where_walk_meets_scan=None if scan_per_query is None or ms_per_row <= 0
                              else int(scan_per_query / ms_per_row)))
                if "host" not in skip:
                    hq = min(args.host_nq, nq)
                    subs = [np.ascontiguousarray(q3[:hq, j]) for j in range(m)]
                    t0 = time.perf_counter()
                    top = host_road(ix, subs, code, ngroups, k)
                    t1 = time.perf_counter()
                    res = ix.search_maxsim(q3[:hq], k, groups)
                    t2 = time.perf_counter()
                    # (the host road sums fp32 scores: the same groups up to near-ties)
                    agree = float(np.mean([len(set(top[a].tolist()) & set(res.keys[a].tolist())) / k for a in range(hq)]))
                    emit(dict(base, what="host", host_nq=hq, host_road_ms_per_query=round((t1 - t0) * 1e3 / hq, 3),
                              maxsim_ms_per_query=round((t2 - t1) * 1e3 / hq, 3), top_k_overlap=round(agree, 4)))
        groups.close()
    ix.close()


if __name__ == "__main__":
    main()

"""Adjusted search: FlatIndex.search_adjusted against the list search it follows, in one process.
Corpus: the bursts of scripts/groups_timing.py (default 100k x 1536, bf16), 256 queries base[:256] + 0.3
noise.  Adjustments: `sparse200` -- 200 random rows with a scale in [0.5, 1.5] and a bonus up to 0.4 (a
keyword store's hits and a few boosted photos: AUTO takes DIRECT) -- and `dense_narrow` -- every row with a
bonus below 0.01 (a recency prior: AUTO takes BOUND).  `--scan` adds each adjustment under the forced SCAN
tier.

Per adjustment and k (10, 100): the library's HIP events (vs_adjust_last_times) split the call into list
search and walk per list tier, the direct scan over the adjusted rows and the full scan; alongside, the
same queries through plain FlatIndex.search at the first list's depth -- that path is untouched by this
feature -- as wall time around the synchronising call, like the whole search_adjusted call.  One untimed
call per shape first; medians over --runs.  One JSON line per shape, also appended to --out.
python scripts/adjust_timing.py [--out profiles/adjust_timing.jsonl] [--n 100000] [--d 1536]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scan", action="store_true")
    args = ap.parse_args()
    n, d = args.n, args.d
    x, q, _ = burst_rows(n, d, 256, 7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 65536):
        ix.add(x[r0:r0 + 65536])
    del x
    rng = np.random.default_rng(11)
    rows = rng.permutation(n)[:200]
    made = {}
    t0 = time.perf_counter()
    made["sparse200"] = ix.score_adjust_sparse(rows, rng.uniform(0.5, 1.5, 200), rng.uniform(0.0, 0.4, 200))
    t1 = time.perf_counter()
    made["dense_narrow"] = ix.score_adjust(None, rng.uniform(0.0, 0.01, n))
    t2 = time.perf_counter()
    create_ms = {"sparse200": (t1 - t0) * 1e3, "dense_narrow": (t2 - t1) * 1e3}
    qq = np.ascontiguousarray(q[:args.nq])
    for name, adj in made.items():
        for mode in ("auto", "scan") if args.scan else ("auto",):
            ix.set_adjust_mode(mode)
            for k in (10, 100):
                L0 = k + min(adj.count, max(k, 64))
                first = None
                wall, plain, ts, tw, td, tf = [], [], [], [], [], []
                for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                    t0 = time.perf_counter()
                    ix.search(qq, L0)
                    t1 = time.perf_counter()
                    res = ix.search_adjusted(qq, k, adj, return_raw=True)
                    t2 = time.perf_counter()
                    t = ix.adjust_last_times()
                    st = ix.adjust_last_stats()
                    if first is None:
                        first = res
                    else:  # the same bits every time
                        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, res))
                    if run:
                        plain.append((t1 - t0) * 1e3)
                        wall.append((t2 - t1) * 1e3)
                        ts.append(t["search_ms"])
                        tw.append(t["walk_ms"])
                        td.append(t["direct_scan_ms"])
                        tf.append(t["full_scan_ms"])
                ts, tw = np.median(np.asarray(ts), axis=0), np.median(np.asarray(tw), axis=0)
                row = {"N": n, "d": d, "dtype": args.dtype, "adjust": name, "adjusted_rows": adj.count,
                       "create_wall_ms": round(create_ms[name], 3), "nq": args.nq, "k": k, "mode": mode, "tier": st["tier"],
                       "L0": L0, "plain_search_L0_wall_ms_median": round(float(np.median(plain)), 3),
                       "adjusted_wall_ms_median": round(float(np.median(wall)), 3),
                       "search_ms_per_tier_median": [round(float(v), 3) for v in ts],
                       "walk_ms_per_tier_median": [round(float(v), 3) for v in tw],
                       "walk_over_search_tier1": round(float(tw[0] / ts[0]), 4) if ts[0] > 0 else None,
                       "direct_scan_ms_median": round(float(np.median(td)), 3),
                       "full_scan_ms_median": round(float(np.median(tf)), 3),
                       "tiers": [st["first"], st["deeper"], st["scan"]], "longest_list": st["longest"],
                       "adjusted_in_top_k_mean": round(float(np.isin(first[1], rows).sum(axis=1).mean()), 2)
                       if name == "sparse200" else None}
                line = json.dumps(row)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a", encoding="utf-8") as f:
                        f.write(line + "\n")
    ix.set_adjust_mode("auto")
    for adj in made.values():
        adj.close()
    ix.close()


if __name__ == "__main__":
    main()

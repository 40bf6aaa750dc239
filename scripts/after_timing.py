"""Paged search: FlatIndex.search_after against what a caller had before it, in one process.
Corpus: the bursts of scripts/groups_timing.py (default 100k x 1536, bf16), 256 queries base[:256] + 0.3
noise.  Pages of 10 and 100 rows at ranks 0, 100 and 1000 under the forced LISTS tier with the true rank hint
(an iterator's call), and at rank 5000 under the forced SCAN tier; the cursor of a page at rank r is the row
ranked r - 1, taken from the library's own ranking.

Per page: wall time around the synchronising call and the library's HIP events (vs_after_last_times: cursor
scoring, list search and cut per list tier, scan).  Alongside, the same page as the parent commit offers it:
plain FlatIndex.search at k = rank + page where that is legal (<= 3276), and the infinite-radius
range_search where it is not -- over --range-nq queries only, since it returns every row of the corpus per
query.  One untimed call per shape first; medians over --runs.  One JSON line per shape, also appended to
--out.
python scripts/after_timing.py [--out profiles/after_timing.jsonl] [--n 100000] [--d 1536]"""
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

KMAX = 3276


def cursor_at(ix, q, rank):
    """after[q] = the row ranked rank - 1 (rank 0: -1), by the library's own ranking."""
    nq = q.shape[0]
    after, at = np.full((nq,), -1, dtype=np.int64), 0
    while at < rank:
        step = min(KMAX, rank - at)
        _, I = ix.search_after(q, step, after, rank_hint=np.full((nq,), at))
        after, at = I[:, step - 1].copy(), at + step
    return after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--range-nq", type=int, default=16)
    args = ap.parse_args()
    n, d = args.n, args.d
    x, q, _ = burst_rows(n, d, 256, 7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 65536):
        ix.add(x[r0:r0 + 65536])
    del x
    qq = np.ascontiguousarray(q[:args.nq])
    for rank, mode in ((0, "lists"), (100, "lists"), (1000, "lists"), (5000, "scan")):
        ix.set_after_mode("auto")
        after = cursor_at(ix, qq, rank)
        hint = np.full((args.nq,), rank, dtype=np.int64)
        for page in (10, 100):
            ix.set_after_mode(mode)
            legal = rank + page <= KMAX
            first = None
            wall, parent, t_score, t_search, t_cut, t_scan = [], [], [], [], [], []
            for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                t0 = time.perf_counter()
                if legal:
                    Dp, Ip = ix.search(qq, rank + page)
                else:
                    lims, Dp, Ip = ix.range_search(qq[:args.range_nq], -np.inf)
                t1 = time.perf_counter()
                res = ix.search_after(qq, page, after, rank_hint=hint, return_rank=True)
                t2 = time.perf_counter()
                t = ix.after_last_times()
                st = ix.after_last_stats()
                if first is None:
                    first = res
                    assert (res[2] == rank).all()
                    if legal:  # the same page, cut from the parent's deeper list
                        assert np.array_equal(Ip[:, rank:], res[1]) and Dp[:, rank:].tobytes() == res[0].tobytes()
                    else:
                        for a in range(args.range_nq):
                            assert np.array_equal(Ip[lims[a] + rank:lims[a] + rank + page], res[1][a])
                else:  # the same bits every time
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, res))
                if run:
                    parent.append((t1 - t0) * 1e3)
                    wall.append((t2 - t1) * 1e3)
                    t_score.append(t["score_ms"])
                    t_search.append(t["search_ms"])
                    t_cut.append(t["cut_ms"])
                    t_scan.append(t["scan_ms"])
            row = {"N": n, "d": d, "dtype": args.dtype, "nq": args.nq, "rank": rank, "page": page, "mode": mode,
                   "after_wall_ms_median": round(float(np.median(wall)), 3),
                   "score_ms_median": round(float(np.median(t_score)), 3),
                   "search_ms_per_tier_median": [round(float(v), 3) for v in np.median(np.asarray(t_search), axis=0)],
                   "cut_ms_per_tier_median": [round(float(v), 3) for v in np.median(np.asarray(t_cut), axis=0)],
                   "scan_ms_median": round(float(np.median(t_scan)), 3),
                   "tiers": [st["first"], st["deeper"], st["scan"]], "longest_list": st["longest"],
                   "parent": f"search k={rank + page}" if legal else "range_search radius=-inf",
                   "parent_nq": args.nq if legal else args.range_nq,
                   "parent_wall_ms_median": round(float(np.median(parent)), 3)}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")
    ix.set_after_mode("auto")
    ix.close()


if __name__ == "__main__":
    main()

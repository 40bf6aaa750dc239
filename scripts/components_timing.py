"""Duplicate groups: FlatIndex.range_components against the roads there were before it, host calls end to
end (each ends in a device synchronise), alternated in one process after a warm-up round.
  new road   range_components(radius): labels, components, edges; nothing per pair leaves the device
  join       range_search_rows(radius, self_mode="above") alone: the pair list the old road starts from
  dup        VectorStore.find_duplicates' own code over that pair list (the dict union-find on the host)
Per store (100k rows, d = 1536; f32 and bf16, the library's own tier) three corpora of the synthetic
generator's unit rows, radius 0.95:
  few     the planted copies of rows_join_timing.py (every 97th row copied over 1-3 successors)
  bursts  1000 groups of 30 near copies (row 100 g and its 29 successors, cos about 0.99 to each other)
  big     20,000 identical rows (2e8 pairs): the join runs once (--no-big-join skips it) and dup is not run
          (2e8 pairs through an interpreted loop)
The groups of the new road are checked against dup's.  Reported: median / minimum wall ms of each road, the
spread (max - min) of the join's repeats, the new road's HIP-event times (vs_components_last_times) and its
stats.  One JSON line per case, also appended to --out.
python scripts/components_timing.py [--out profiles/components_timing.jsonl] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402
from photo_search_engine_amd.vector_store import VectorStore  # noqa: E402

STORES = [(100_000, 1536, "f32"), (100_000, 1536, "bf16")]
RADIUS = 0.95


class PairSource:
    """What VectorStore.find_duplicates reads of its store: duplicate_pairs over a FlatIndex."""

    def __init__(self, ix):
        self.ix = ix

    def duplicate_pairs(self, threshold, allowed=None):
        lims, distances, indices = self.ix.range_search_rows(float(threshold), self_mode="above")
        return np.repeat(np.arange(self.ix.ntotal, dtype=np.int64), np.diff(lims)), indices, distances


def groups_of(labels):
    order = np.argsort(labels, kind="stable")
    starts = np.flatnonzero(np.diff(labels[order], prepend=-1))
    return [g.tolist() for g in np.split(order, starts[1:]) if g.shape[0] >= 2]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def alternate_ms(fns, reps, warm=1):
    outs = [None] * len(fns)
    for _ in range(warm):
        for i, fn in enumerate(fns):
            outs[i] = fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t, outs[i] = timed(fn)
            ts[i].append(t)
    return ts, outs


def summary(t):
    return {"median_ms": round(float(np.median(t)), 2), "min_ms": round(float(np.min(t)), 2),
            "spread_ms": round(float(np.max(t) - np.min(t)), 2)}


def plant(x, case, rng):
    N, d = x.shape
    if case == "few":
        for base in range(0, N - 4, 97):
            for c in range(1 + base % 3):
                x[base + 1 + c] = x[base]
    elif case == "bursts":
        for g in range(min(1000, N // 100)):
            rows = x[100 * g] + (0.1 / np.sqrt(d)) * rng.standard_normal((30, d)).astype(np.float32)
            x[100 * g:100 * g + 30] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    else:
        x[2 * N // 5:3 * N // 5] = x[2 * N // 5]


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="20k rows, fewer repetitions")
    ap.add_argument("--no-big-join", action="store_true", help="do not run the self-join of the big group")
    ap.add_argument("--cases", default="few,bursts,big")
    ap.add_argument("--dtypes", default="f32,bf16")
    args = ap.parse_args()
    for N, d, dtype in STORES:
        if dtype not in args.dtypes.split(","):
            continue
        if args.quick:
            N = 20_000
        reps = 2 if args.quick else 5
        for case in args.cases.split(","):
            x = O.synth_rows(O.SEED_CORPUS, 0, N, d, True, "f32")
            plant(x, case, np.random.default_rng(11))
            ix = FlatIndex(d, "ip", dtype)
            ix.add(x)
            del x
            src = PairSource(ix)
            new = lambda: ix.range_components(RADIUS)  # noqa: E731
            join = lambda: ix.range_search_rows(RADIUS, self_mode="above")  # noqa: E731
            dup = lambda: VectorStore.find_duplicates(src, RADIUS)  # noqa: E731
            row = {"case": case, "N": N, "d": d, "dtype": dtype, "radius": RADIUS}
            if case != "big":
                ts, (res_new, res_join, res_dup) = alternate_ms([new, join, dup], reps)
                row.update(new=summary(ts[0]), join=summary(ts[1]), dup=summary(ts[2]),
                           join_tier=ix.range_last_stats()["tier"], join_rescanned=ix.range_last_stats()["rescanned"],
                           pairs=int(res_join[0][-1]), same_groups=bool(groups_of(res_new[0]) == res_dup),
                           same_edges=bool(res_new[2] == int(res_join[0][-1])))
                row["new_minus_join_ms"] = round(row["new"]["median_ms"] - row["join"]["median_ms"], 2)
                row["join_over_new"] = round(row["join"]["median_ms"] / row["new"]["median_ms"], 3)
                row["dup_over_new"] = round(row["dup"]["median_ms"] / row["new"]["median_ms"], 3)
            else:
                ts, (res_new,) = alternate_ms([new], 3 if not args.quick else 2)
                row.update(new=summary(ts[0]))
                m = N // 5
                row["expected"] = bool(res_new[2] >= m * (m - 1) // 2 and
                                       (res_new[0][2 * N // 5:3 * N // 5] == 2 * N // 5).all())
                if not args.no_big_join:
                    try:
                        t, res_join = timed(join)
                        row["join_once_ms"] = round(t, 2)
                        row["pairs"] = int(res_join[0][-1])
                        row["same_edges"] = bool(res_new[2] == row["pairs"])
                        row["join_host_sorted"] = ix.range_last_stats()["host_sorted"]
                        row["join_result_bytes"] = int(sum(a.nbytes for a in res_join))
                        row["join_over_new"] = round(t / row["new"]["median_ms"], 3)
                        del res_join
                    except (MemoryError, RuntimeError) as e:
                        row["join_error"] = str(e)[:200]
                row["dup"] = "not run: 2e8 pairs through the host union-find's interpreted loop"
            st, tm = ix.components_last_stats(), ix.components_last_times()
            row.update(components=res_new[1], edges=res_new[2], tier=st["tier"], rescanned=st["rescanned"],
                       blocks=st["blocks"], screen_ms=round(tm["screen_ms"], 3), scan_ms=round(tm["scan_ms"], 3),
                       readback_ms=round(tm["readback_ms"], 3))
            emit(row, args.out)
            ix.close()


if __name__ == "__main__":
    main()

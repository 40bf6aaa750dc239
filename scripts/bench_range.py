"""Range search against what a user does without it, host calls end to end (wall medians around calls
that end in a device synchronise, after warm-up; legs alternate inside every repetition).  Per setting:
  (a) FlatIndex.range_search forced to the scan tier,
  (b) the same forced to the screen tier, where it applies (bf16 / f16 rows, 9..256 queries),
  (c) today's method on the same build: search(q, k) at k = the largest per-query count, then a host
      cut at the radius -- the top-k path, which range search does not touch.
The radii are each query's 101st-best D, so every query returns 100 rows; (a), (b) and (c) are
compared bit for bit.  One JSON line per setting, also appended to --out.
  --only LEG runs one leg alone a few times (scan | screen | topk), for a kernel trace of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_range.py --setting 0 --only screen
python scripts/bench_range.py [--out profiles/bench_range.jsonl] [--setting 0|1] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402

SETTINGS = [(1_000_000, 1536, "bf16", 256), (100_000, 4096, "f32", 1)]  # the scale shape; the product's call
QUICK = [(50_000, 256, "bf16", 256), (20_000, 512, "f32", 1)]
RESULTS = 100


def topk_cut(ix, q, radius, k):
    D, I = ix.search(q, k)
    keep = D > radius[:, None]  # (inner product)
    lims = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return lims, D[keep], I[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--setting", type=int, default=None)
    ap.add_argument("--only", choices=["scan", "screen", "topk"], default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    settings = QUICK if args.quick else SETTINGS
    for si, (N, d, dtype, nq) in enumerate(settings):
        if args.setting is not None and si != args.setting:
            continue
        ix = FlatIndex(d, "ip", dtype)
        ix.add_synthetic(O.SEED_CORPUS, 0, N, True)
        q = O.synth_rows(O.SEED_QUERIES, 0, nq, d, True, "f32")
        D, _ = ix.search(q, RESULTS + 1)
        radius = np.ascontiguousarray(D[:, RESULTS])
        legs = {}
        for mode in ("scan", "screen"):
            if mode == "screen" and not (dtype in ("bf16", "f16") and 9 <= nq <= 256):
                continue

            def leg(mode=mode):
                ix.set_range_mode(mode)
                return ix.range_search(q, radius)
            legs[mode] = leg
        k = None

        def topk():
            return topk_cut(ix, q, radius, k)
        legs["topk"] = topk
        if args.only:
            legs = {args.only: legs[args.only]} if args.only in legs else {}
        out, times = {}, {name: [] for name in legs}
        lims = ix.range_search(q, radius)[0]
        k = int(np.diff(lims).max())
        for name, fn in legs.items():  # warm-up: every shape the timed window uses
            for _ in range(2):
                out[name] = fn()
        for _ in range(args.reps):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                out[name] = fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"N": N, "d": d, "dtype": dtype, "nq": nq, "results_per_query": float(np.diff(lims).mean()), "k": k}
        for name in legs:
            row[name] = {"median_ms": round(float(np.median(times[name])), 4), "min_ms": round(float(np.min(times[name])), 4),
                         "max_ms": round(float(np.max(times[name])), 4)}
            if name != "topk":
                ix.set_range_mode(name)
                ix.range_search(q, radius)
                st = ix.range_last_stats()
                row[name].update(tier=st["tier"], rescanned=st["rescanned"])
        names = list(out)
        row["identical"] = all(np.array_equal(a, b) for n in names[1:] for a, b in zip(out[names[0]], out[n]))
        ix.set_range_mode("auto")
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
        ix.close()


if __name__ == "__main__":
    main()

"""Diversified search: FlatIndex.search_diverse against the plain search it follows, in one process.
Corpus: bursts built on the host with the recipe of tests/test_gpu_diverse.py scaled up -- base vectors
standard_normal(d), burst b of 1 + (5 b) % 12 members base[b] + 0.05 noise, shuffled, unit-normalised,
cut at N rows (default 100k x 1536, bf16); queries base[:256] + 0.3 noise.  The cosine threshold 0.9
lies inside the burst gap (burst members score ~0.9975 with each other, different bursts ~0).

Per shape (batch 1 and 256; k = 10 and 100): the library's HIP events (vs_diverse_last_times) split
the call into the list search and the walk of each tier; alongside, the same queries through plain
FlatIndex.search at the first list's depth L0 = max(4 k, 64) -- that path is untouched by this
feature -- as wall time around the synchronising call, like the whole search_diverse call.  One untimed
call per shape first; medians over --runs.  Reported: the tier-1 walk as a multiple of the tier-1 list
search, examined per query (mean / max) and the tier counts.  One JSON line per shape, also appended
to --out.
python scripts/diverse_timing.py [--out profiles/diverse_timing.jsonl] [--n 100000] [--d 1536]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from photo_search_engine_amd.index import FlatIndex  # noqa: E402


def burst_rows(n, d, nq, seed):
    rng = np.random.default_rng(seed)
    nbase = n // 6 + nq + 16  # (bursts average 6.5 rows: enough bases for n rows)
    base = rng.standard_normal((nbase, d)).astype(np.float32)
    sizes = 1 + (5 * np.arange(nbase)) % 12
    owner = np.repeat(np.arange(nbase), sizes)[:n]
    assert owner.shape[0] == n
    x = np.empty((n, d), dtype=np.float32)
    for r0 in range(0, n, 8192):  # (chunks: the noise of 100k x 1536 rows at once is 1.2 GB of fp64)
        o = owner[r0:r0 + 8192]
        x[r0:r0 + 8192] = base[o] + np.float32(0.05) * rng.standard_normal((o.shape[0], d)).astype(np.float32)
    rng.shuffle(x)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = base[:nq] + np.float32(0.3) * rng.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return x, np.ascontiguousarray(q, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    n, d = args.n, args.d
    x, q = burst_rows(n, d, 256, 7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 65536):
        ix.add(x[r0:r0 + 65536])
    del x
    for nq in (1, 256):
        for k in (10, 100):
            qq = np.ascontiguousarray(q[:nq])
            L0 = max(4 * k, 64)
            first = None
            wall, plain, ts, tw = [], [], [], []
            for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                t0 = time.perf_counter()
                Dp, Ip = ix.search(qq, L0)
                t1 = time.perf_counter()
                res = ix.search_diverse(qq, k, args.threshold)
                t2 = time.perf_counter()
                t = ix.diverse_last_times()
                st = ix.diverse_last_stats()
                if first is None:
                    first = res
                    assert (res.hidden.sum(axis=1) + (res.I >= 0).sum(axis=1) == res.examined).all()
                else:  # the same bits every time
                    assert first.I.tobytes() == res.I.tobytes() and first.hidden.tobytes() == res.hidden.tobytes()
                if run:
                    plain.append((t1 - t0) * 1e3)
                    wall.append((t2 - t1) * 1e3)
                    ts.append(t["search_ms"])
                    tw.append(t["walk_ms"])
            ts, tw = np.median(np.asarray(ts), axis=0), np.median(np.asarray(tw), axis=0)
            row = {"N": n, "d": d, "dtype": args.dtype, "threshold": args.threshold, "nq": nq, "k": k, "L0": L0,
                   "plain_search_L0_wall_ms_median": round(float(np.median(plain)), 3),
                   "diverse_wall_ms_median": round(float(np.median(wall)), 3),
                   "search_ms_per_tier_median": [round(float(v), 3) for v in ts],
                   "walk_ms_per_tier_median": [round(float(v), 3) for v in tw],
                   "walk_over_search_tier1": round(float(tw[0] / ts[0]), 3) if ts[0] > 0 else None,
                   "examined_mean": round(float(first.examined.mean()), 1), "examined_max": int(first.examined.max()),
                   "accepted_min": int((first.I >= 0).sum(axis=1).min()),
                   "tiers": [st["first"], st["deeper"], st["full"]], "longest_list": st["longest"]}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")
    ix.close()


if __name__ == "__main__":
    main()

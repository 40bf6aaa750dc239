"""Grouped search: FlatIndex.search_groups against the plain search it follows, in one process.
Corpus: the bursts of scripts/diverse_timing.py (base vectors standard_normal(d), burst b of 1 + (5 b) % 12
members base[b] + 0.05 noise, unit-normalised, cut at N rows; default 100k x 1536, bf16) with the burst id
shuffled alongside the rows so it survives as a key; queries base[:256] + 0.3 noise.  Keys: `burst` (about
N / 6.5 small groups whose members score alike, so a group's rows sit together in a ranking) and `id % 12`
(twelve groups of N / 12 rows spread evenly through every ranking).

Per shape (batch 1 and 256; (k, g) = (10, 1) and (10, 3)) and depth setting -- the defaults, and
(k g, k g), the smallest legal lists, which pushes queries into the restricted rounds so that a round's
cost can be read: the library's HIP events (vs_group_last_times) split the call into list search and walk
per tier, and the rounds' list search further into building the restricted set, compacting it and the
scan; alongside, the same queries through plain FlatIndex.search at the first list's depth L0 =
max(4 k g, 64) -- that path is untouched by this feature -- as wall time around the synchronising call,
like the whole search_groups call.  One untimed call per shape first; medians over --runs.  One JSON line
per shape and depth, also appended to --out.
python scripts/groups_timing.py [--out profiles/groups_timing.jsonl] [--n 100000] [--d 1536]"""
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
    owner = owner[rng.permutation(n)]  # (the burst id rides the shuffle)
    x = np.empty((n, d), dtype=np.float32)
    for r0 in range(0, n, 8192):  # (chunks: the noise of 100k x 1536 rows at once is 1.2 GB of fp64)
        o = owner[r0:r0 + 8192]
        x[r0:r0 + 8192] = base[o] + np.float32(0.05) * rng.standard_normal((o.shape[0], d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = base[:nq] + np.float32(0.3) * rng.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return x, np.ascontiguousarray(q, dtype=np.float32), owner.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    n, d = args.n, args.d
    x, q, owner = burst_rows(n, d, 256, 7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 65536):
        ix.add(x[r0:r0 + 65536])
    del x
    schemes = {"burst": owner, "id%12": np.arange(n, dtype=np.int64) % 12}
    for name, keys in schemes.items():
        t0 = time.perf_counter()
        groups = ix.group_keys(keys)
        create_ms = (time.perf_counter() - t0) * 1e3
        for nq in (1, 256):
            for k, g in ((10, 1), (10, 3)):
                qq = np.ascontiguousarray(q[:nq])
                L0 = max(4 * k * g, 64)
                for depth in ((0, 0), (k * g, k * g)):
                    ix.set_group_depth(*depth)
                    first = None
                    wall, plain, ts, tw, tr, tc = [], [], [], [], [], []
                    for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                        t0 = time.perf_counter()
                        ix.search(qq, L0)
                        t1 = time.perf_counter()
                        res = ix.search_groups(qq, k, groups, g)
                        t2 = time.perf_counter()
                        t = ix.group_last_times()
                        st = ix.group_last_stats()
                        if first is None:
                            first = res
                        else:  # the same bits every time
                            assert first.I.tobytes() == res.I.tobytes() and first.keys.tobytes() == res.keys.tobytes()
                        if run:
                            plain.append((t1 - t0) * 1e3)
                            wall.append((t2 - t1) * 1e3)
                            ts.append(t["search_ms"])
                            tw.append(t["walk_ms"])
                            tr.append(t["restrict_ms"])
                            tc.append(t["compact_ms"])
                    ts, tw = np.median(np.asarray(ts), axis=0), np.median(np.asarray(tw), axis=0)
                    tr, tc = float(np.median(tr)), float(np.median(tc))
                    rounds = st["rounds"]
                    per_round = None
                    if rounds:  # one restricted round: build R, compact, scan, walk
                        per_round = {"restrict_ms": round(tr / rounds, 4), "compact_ms": round(tc / rounds, 4),
                                     "scan_ms": round((float(ts[2]) - tr - tc) / rounds, 4),
                                     "walk_ms": round(float(tw[2]) / rounds, 4)}
                    row = {"N": n, "d": d, "dtype": args.dtype, "keys": name, "groups": groups.count,
                           "groups_create_wall_ms": round(create_ms, 3), "nq": nq, "k": k, "g": g, "depth": list(depth),
                           "L0": L0, "plain_search_L0_wall_ms_median": round(float(np.median(plain)), 3),
                           "groups_wall_ms_median": round(float(np.median(wall)), 3),
                           "search_ms_per_tier_median": [round(float(v), 3) for v in ts],
                           "walk_ms_per_tier_median": [round(float(v), 3) for v in tw],
                           "walk_over_search_tier1": round(float(tw[0] / ts[0]), 4) if ts[0] > 0 else None,
                           "tiers": [st["first"], st["deeper"], st["finished"]], "rounds": rounds,
                           "per_round_ms": per_round, "longest_list": st["longest"],
                           "groups_returned_min": int((first.found > 0).sum(axis=1).min())}
                    line = json.dumps(row)
                    print(line, flush=True)
                    if args.out:
                        with open(args.out, "a", encoding="utf-8") as f:
                            f.write(line + "\n")
        groups.close()
    ix.set_group_depth(0, 0)
    ix.close()


if __name__ == "__main__":
    main()

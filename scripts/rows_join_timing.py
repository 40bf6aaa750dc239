"""Queries taken from stored rows: what keeping them on the device buys, host calls end to end (each ends
in a device synchronise).  Per store (100k rows, d = 1536; f32 and bf16) the median and minimum wall ms of
  (a) the exact kNN graph of every row at k = 64:  FlatIndex.search_rows(all ids, 64)  against the route
      VectorStore._knn_graph takes today -- reconstruct_n of 4096 rows to the host, search at k + 1,
      the row itself dropped with numpy -- with the two id arrays compared bit for bit;
  (b) the whole-corpus range join, range_search_rows(radius) under self_mode "above" against "drop",
      on the scan tier (f32) and the screen tier (bf16); the pair sets are compared.
The corpus is the synthetic generator's unit rows with planted near-duplicate groups (a row copied over
its successors, every 97th row, 1-3 copies), the radius 0.95.  The two versions of each comparison run
alternately in one process, warmed up first.  One JSON line per case, also appended to --out.
python scripts/rows_join_timing.py [--out profiles/rows_join_timing.jsonl] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402

STORES = [(100_000, 1536, "f32"), (100_000, 1536, "bf16")]
K = 64
RADIUS = 0.95


def alternate_ms(fns, reps, warm=1):
    """Median / minimum wall ms of each callable, run alternately (warm-up rounds first); last outputs."""
    outs = [None] * len(fns)
    for _ in range(warm):
        for i, fn in enumerate(fns):
            outs[i] = fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            outs[i] = fn()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(t)), float(np.min(t))) for t in ts], outs


def knn_host_route(ix, k):
    """VectorStore._knn_graph's loop: every row crosses the host twice."""
    n = ix.ntotal
    out = np.full((n, k), -1, dtype=np.int64)
    for r0 in range(0, n, 4096):
        rows = ix.reconstruct_n(r0, min(4096, n - r0))
        _, I = ix.search(rows, min(n, k + 1))
        own = np.arange(r0, r0 + I.shape[0])[:, None]
        ok = (I >= 0) & (I != own)
        pos = np.cumsum(ok, axis=1) - 1
        ok &= pos < k
        r, c = np.nonzero(ok)
        out[r0 + r, pos[r, c]] = I[r, c]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="20k rows, fewer repetitions")
    args = ap.parse_args()
    for N, d, dtype in STORES:
        if args.quick:
            N = 20_000
        x = O.synth_rows(O.SEED_CORPUS, 0, N, d, True, "f32")
        planted = 0
        for base in range(0, N - 4, 97):
            for c in range(1 + base % 3):
                x[base + 1 + c] = x[base]
                planted += 1
        ix = FlatIndex(d, "ip", dtype)
        ix.add(x)
        del x
        ids = np.arange(N, dtype=np.int64)
        reps = 2 if args.quick else 5

        (dev, host), (res_dev, res_host) = alternate_ms(
            [lambda: ix.search_rows(ids, K)[1], lambda: knn_host_route(ix, K)], reps)
        row = {"case": "knn_graph", "N": N, "d": d, "dtype": dtype, "k": K,
               "search_rows": {"median_ms": round(dev[0], 2), "min_ms": round(dev[1], 2)},
               "host_route": {"median_ms": round(host[0], 2), "min_ms": round(host[1], 2)},
               "identical_ids": bool(np.array_equal(res_dev, res_host)),
               # the host route's own copies, timed apart: rows to the host and back as queries
               "pcie_bytes_host_route": 2 * N * d * 4}
        t0 = time.perf_counter()
        for r0 in range(0, N, 4096):
            ix.reconstruct_n(r0, min(4096, N - r0))
        row["reconstruct_only_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        emit(row, args.out)

        for tier in ("scan", "screen") if dtype != "f32" else ("scan",):
            ix.set_range_mode(tier)
            (ab, dr), (res_a, res_d) = alternate_ms(
                [lambda: ix.range_search_rows(RADIUS, self_mode="above"),
                 lambda: ix.range_search_rows(RADIUS, self_mode="drop")], reps)
            st = ix.range_last_stats()
            qa = np.repeat(ids, np.diff(res_a[0]))
            qd = np.repeat(ids, np.diff(res_d[0]))
            up = res_d[2] > qd
            emit({"case": "range_join", "N": N, "d": d, "dtype": dtype, "tier": tier, "tier_taken": st["tier"],
                  "radius": RADIUS, "pairs_above": int(res_a[0][-1]), "entries_drop": int(res_d[0][-1]),
                  "planted_copies": planted,
                  "above": {"median_ms": round(ab[0], 2), "min_ms": round(ab[1], 2)},
                  "drop": {"median_ms": round(dr[0], 2), "min_ms": round(dr[1], 2)},
                  "above_over_drop": round(ab[0] / dr[0], 3),
                  "same_pairs": bool(np.array_equal(qa, qd[up]) and np.array_equal(res_a[2], res_d[2][up])),
                  "rescanned": st["rescanned"]}, args.out)
        ix.set_range_mode("auto")
        ix.close()


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Filtered search: the two tiers of vs_search_sel against the reference's own method, host calls end to
end.  Per case (store, selectivity, nq; k = 10) the median wall ms of
  (a) FlatIndex.search(q, k, sel=selector) forced to the scan tier,
  (b) the same forced to the overfetch tier (with the queries the scan had to re-answer),
  (c) the reference's method through the existing API: an unfiltered search at the inflated
      candidate_k of searcher._calculate_candidate_k (500 for stores this large at top_k 10 with a
      time filter, first round) and a numpy post-filter -- with how many queries it left short of k.
(a) and (b) are compared bit for bit.  One JSON line per case, also appended to --out.
python scripts/sel_scan_timing.py [--out profiles/sel_scan_timing.jsonl] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402

STORES = [(100_000, 1536, "f32"), (1_000_000, 1536, "bf16")]  # the product shape; the scale shape
SELECTIVITY = [0.001, 0.01, 0.1, 0.5]
NQ = [1, 256]
K = 10
CANDIDATE_K = 500


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the first store only, fewer repetitions")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    for N, d, dtype in STORES[:1] if args.quick else STORES:
        ix = FlatIndex(d, "ip", dtype)
        ix.add_synthetic(O.SEED_CORPUS, 0, N, True)
        for frac in SELECTIVITY:
            mask = rng.random(N) < frac
            sel = ix.selector(mask)
            for nq in NQ:
                q = O.synth_rows(O.SEED_QUERIES, 0, nq, d, True, "f32")
                reps = (30 if nq == 1 else 5) // (3 if args.quick else 1) + 1
                row = {"N": N, "d": d, "dtype": dtype, "selectivity": frac, "m": sel.count, "nq": nq, "k": K}
                res = {}
                for mode in ("scan", "overfetch"):
                    ix.set_sel_mode(mode)
                    med, lo, res[mode] = median_ms(lambda: ix.search(q, K, sel=sel), reps)
                    st = ix.sel_last_stats()
                    row[mode] = {"median_ms": round(med, 4), "min_ms": round(lo, 4), "kprime": st["kprime"],
                                 "rescanned": st["rescanned"]}
                    if mode == "scan":
                        row[mode]["gather_GBps"] = round(nq * sel.count * d * (4 if dtype == "f32" else 2) / med / 1e6, 1)
                ix.set_sel_mode("auto")
                ix.search(q, K, sel=sel)
                row["auto_tier"] = ix.sel_last_stats()["tier"]
                row["identical"] = bool(np.array_equal(res["scan"][0], res["overfetch"][0])
                                        and np.array_equal(res["scan"][1], res["overfetch"][1]))

                def reference_method():
                    _, I = ix.search(q, CANDIDATE_K)
                    keep = mask[I]
                    return [I[a][keep[a]][:K] for a in range(nq)]

                med, lo, kept = median_ms(reference_method, reps)
                row["postfilter"] = {"candidate_k": CANDIDATE_K, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                                     "queries_short_of_k": int(sum(len(r) < min(K, sel.count) for r in kept))}
                line = json.dumps(row)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a", encoding="utf-8") as f:
                        f.write(line + "\n")
            sel.close()
        ix.close()


if __name__ == "__main__":
    main()

"""Facet counts: FlatIndex.range_count against the only exact road there was before it, range_search +
np.bincount of the keys on the host, in one process on the same inputs.
Corpus: standard_normal rows, unit-normalised (default 100k x 1536, bf16), 256 queries of the same kind.
Radii: each query's own score at rank 10 and at rank 1000 (from one plain search), and -inf (every row).
Keys: G = 12, 365 and 50,000 uniformly drawn groups (the last is past VS_FACET_LDS_BINS: global form only).

Per radius, G, tier (scan, screen) and histogram form (auto, and the forced lds / global pair behind the
AUTO rule): wall time around the synchronising range_count call and the library's HIP events
(vs_facet_last_times: screen + refine, scan, table readback); per radius and tier, once, the baseline:
wall time of range_search plus the bincount over its ids.  The counts of every form are checked against
the baseline's.  One untimed call first; medians over --runs (the baseline at -inf, 25.6 M rows through the
host sort, runs --runs-inf times).  One JSON line per measurement, also appended to --out.
python scripts/facet_timing.py [--out profiles/facet_timing.jsonl] [--n 100000] [--d 1536]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from photo_search_engine_amd.index import FACET_LDS_BINS, FlatIndex  # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--runs-inf", type=int, default=1)
    ap.add_argument("--groups", default="12,365,50000")
    args = ap.parse_args()
    n, d, nq = args.n, args.d, args.nq
    rng = np.random.default_rng(7)
    ix = FlatIndex(d, "ip", args.dtype)
    for r0 in range(0, n, 8192):
        x = rng.standard_normal((min(8192, n - r0), d)).astype(np.float32)
        ix.add(x / np.linalg.norm(x, axis=1, keepdims=True))
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    D, _ = ix.search(q, min(1000, n))
    radii = {"rank10": D[:, 9].copy(), "rank1000": D[:, -1].copy(), "inf": np.full((nq,), -np.inf, dtype=np.float32)}
    key_sets = {G: rng.integers(0, G, n).astype(np.int64) for G in (int(g) for g in args.groups.split(","))}
    for rname, r in radii.items():
        for tier in ("scan", "screen"):
            ix.set_range_mode(tier)
            # the baseline: range_search, then one bincount per key set on the host
            wall, I, lims = [], None, None
            for run in range((args.runs_inf if rname == "inf" else args.runs) + 1):  # (run 0: warm-up)
                t0 = time.perf_counter()
                lims, _, I = ix.range_search(q, r)
                t1 = time.perf_counter()
                if run or rname == "inf":
                    wall.append((t1 - t0) * 1e3)
            st = ix.range_last_stats()
            base = {"N": n, "d": d, "dtype": args.dtype, "nq": nq, "radius": rname, "tier": tier,
                    "results": int(lims[-1]), "range_search_wall_ms_median": round(float(np.median(wall)), 3),
                    "range_tier": st["tier"], "range_rescanned": st["rescanned"], "range_host_sorted": st["host_sorted"]}
            for G, keys in key_sets.items():
                t0 = time.perf_counter()
                want = np.stack([np.bincount(keys[I[lims[i]:lims[i + 1]]], minlength=G + 1) for i in range(nq)])
                bincount_ms = (time.perf_counter() - t0) * 1e3
                groups = ix.group_keys(keys)
                for form in ("auto", "lds", "global") if groups.count + 1 <= FACET_LDS_BINS else ("auto", "global"):
                    ix.set_facet_hist(form)
                    wall, ev = [], []
                    for run in range(args.runs + 1):
                        t0 = time.perf_counter()
                        totals, counts = ix.range_count(q, r, groups=groups)
                        t1 = time.perf_counter()
                        if run:
                            wall.append((t1 - t0) * 1e3)
                            t = ix.facet_last_times()
                            ev.append([t["screen_ms"], t["scan_ms"], t["readback_ms"]])
                    assert np.array_equal(counts[:, :groups.count], want[:, groups.keys]) and not counts[:, -1].any()
                    assert np.array_equal(totals, np.diff(lims))
                    fs = ix.facet_last_stats()
                    ev = np.median(np.asarray(ev), axis=0)
                    emit(dict(base, G=groups.count, form=form, form_taken=fs["hist"], count_tier=fs["tier"],
                              count_rescanned=fs["rescanned"], bincount_wall_ms=round(bincount_ms, 3),
                              range_count_wall_ms_median=round(float(np.median(wall)), 3),
                              screen_ms=round(float(ev[0]), 3), scan_ms=round(float(ev[1]), 3),
                              readback_ms=round(float(ev[2]), 3),
                              baseline_over_count=round((base["range_search_wall_ms_median"] + bincount_ms)
                                                        / float(np.median(wall)), 2)), args.out)
                ix.set_facet_hist("auto")
                groups.close()
    ix.set_range_mode("auto")
    ix.close()


if __name__ == "__main__":
    main()

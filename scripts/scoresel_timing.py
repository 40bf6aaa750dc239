"""Score selectors: FlatIndex.selector_from_range against the only road there was before it, range_search ->
host mask -> selector(mask), in one process on the same inputs; and its kernels against the facet counts'
(range_count without groups: the same scan and refine with the histogram sink) at the same shapes.
Corpus: standard_normal rows, unit-normalised (100k x 1536; bf16 and f32), queries of the same kind.
Radii: each query's own score at rank 10 and at rank 1000 (from one plain search), and -inf (every row).
nq 1, 16, 256; modes any, all; range mode auto and scan.

Per case: wall ms around the call that leaves a selector ready to use (new road; old road) and the library's
HIP events (vs_scoresel_last_times: screen + refine, scan + fold, finish; vs_facet_last_times for
range_count).  The bitmaps of both roads are compared.  One untimed call first; medians over --runs (the old
road at -inf with 256 queries, 25.6 M pairs through the host sort, runs once), and the spread (max - min)
of the facet kernels' time over the runs.  One JSON line per measurement, also appended to --out.

The driver starts one child process per dtype, each under its own time limit, and stops at the first that
fails or runs out of time.
python scripts/scoresel_timing.py [--out profiles/scoresel_timing.jsonl] [--n 100000] [--d 1536]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


def worker(args, dtype):
    from photo_search_engine_amd.index import FlatIndex
    n, d = args.n, args.d
    rng = np.random.default_rng(7)
    ix = FlatIndex(d, "ip", dtype)
    for r0 in range(0, n, 8192):
        x = rng.standard_normal((min(8192, n - r0), d)).astype(np.float32)
        ix.add(x / np.linalg.norm(x, axis=1, keepdims=True))
    qall = rng.standard_normal((256, d)).astype(np.float32)
    qall /= np.linalg.norm(qall, axis=1, keepdims=True)
    Dall, _ = ix.search(qall, min(1000, n))
    for nq in (1, 16, 256):
        q, D = qall[:nq], Dall[:nq]
        radii = {"rank10": D[:, 9].copy(), "rank1000": D[:, -1].copy(), "inf": np.full((nq,), -np.inf, dtype=np.float32)}
        for rname, r in radii.items():
            # the old road's first half is the same for both modes
            heavy = rname == "inf" and nq == 256
            for mode in ("any", "all"):
                def old_road():
                    lims, _, I = ix.range_search(q, r)
                    hits = np.bincount(I, minlength=n)
                    s = ix.selector(hits > 0 if mode == "any" else hits == nq)
                    return s, int(lims[-1])

                wall_old, pairs, want = [], 0, None
                for run in range((1 if heavy else args.runs) + 1):  # (run 0: warm-up; timed too when it is the only other)
                    t0 = time.perf_counter()
                    s, pairs = old_road()
                    t1 = time.perf_counter()
                    if run or heavy:
                        wall_old.append((t1 - t0) * 1e3)
                    want = s.bitmap.copy()
                    s.close()
                for tier in ("auto", "scan"):
                    ix.set_range_mode(tier)
                    wall, ev, m = [], [], 0
                    for run in range(args.runs + 1):
                        t0 = time.perf_counter()
                        s = ix.selector_from_range(q, r, mode=mode)
                        t1 = time.perf_counter()
                        if run:
                            wall.append((t1 - t0) * 1e3)
                            t = ix.scoresel_last_times()
                            ev.append([t["screen_ms"], t["scan_ms"], t["finish_ms"]])
                        else:
                            assert np.array_equal(s.bitmap, want), (dtype, nq, rname, mode, tier)
                        m = s.count
                        s.close()
                    st = ix.scoresel_last_stats()
                    # the facet counts at the same shape and tier: the same kernels with the histogram sink
                    fev = []
                    for run in range(args.runs + 1):
                        ix.range_count(q, r)
                        if run:
                            t = ix.facet_last_times()
                            fev.append(t["screen_ms"] + t["scan_ms"])
                    fs = ix.facet_last_stats()
                    ev = np.median(np.asarray(ev), axis=0)
                    new_ms, old_ms = float(np.median(wall)), float(np.median(wall_old))
                    emit({"N": n, "d": d, "dtype": dtype, "nq": nq, "radius": rname, "mode": mode, "range_mode": tier,
                          "m": m, "pairs_old_road": pairs, "tier": st["tier"], "rescanned": st["rescanned"],
                          "blocks": st["blocks"], "new_wall_ms_median": round(new_ms, 3),
                          "old_wall_ms_median": round(old_ms, 3), "old_over_new": round(old_ms / new_ms, 2),
                          "screen_ms": round(float(ev[0]), 3), "scan_ms": round(float(ev[1]), 3),
                          "finish_ms": round(float(ev[2]), 3), "kernels_ms": round(float(ev[0] + ev[1]), 3),
                          "facet_kernels_ms_median": round(float(np.median(fev)), 3),
                          "facet_kernels_ms_spread": round(float(np.max(fev) - np.min(fev)), 3),
                          "facet_tier": fs["tier"], "facet_rescanned": fs["rescanned"]}, args.out)
                ix.set_range_mode("auto")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one dtype's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args, args.worker)
        return 0
    for dtype in args.dtypes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", dtype, "--n", str(args.n), "--d", str(args.d),
               "--runs", str(args.runs)] + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"scoresel_timing: the {dtype} step ran past {args.step_timeout} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:  # nothing more is started after a step that failed
            print(f"scoresel_timing: the {dtype} step ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

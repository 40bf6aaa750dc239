"""Row removal: vs_remove_ids against the only alternative there was before it, reset() + add() of
the survivors from host memory, in one process.  Index: N rows of d (default 1M x 1536, bf16, inner
product), with the int8 screen (the product's default: the removal moves the rows and requantises
them) and with the native screen (the move alone).  Cases: a random 1 %, the first 10 % as a block,
the last row only.  Per case the median wall ms of FlatIndex.remove_ids over --runs freshly built
indexes (one untimed run first; the call ends in a device synchronise), the bytes of the rows that
move and the HBM traffic the design predicts for them -- each moved row read twice and written twice
(gather into the bounce buffer, place), plus the requantise pass over the rows from the first removed
row's group on (stored row read for the group means and again for the codes, int8 row written) --
with the rate that traffic implies, to hold against the ~6.3 TB/s a streaming copy achieves.
One JSON line per case, also appended to --out.
python scripts/remove_timing.py [--out profiles/remove_timing.jsonl] [--n 1000000] [--d 1536]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402

TR, GROUP = 256, 4096


def build(n, d, dtype, screen):
    ix = FlatIndex(d, "ip", dtype)
    ix.set_screen(screen)
    ix.add_synthetic(O.SEED_CORPUS, 0, n, True)
    return ix


def traffic(n, d, dtype, screen, mask):
    """(moved bytes, predicted HBM bytes) of a removal, from the shapes alone."""
    es = 4 if dtype == "f32" else 2
    dpad = max(-(-d // (128 // es)) * (128 // es), 64)
    row = dpad * es + 4  # stored row + its sqn entry
    f = int(np.argmax(mask))
    n_new = n - int(mask.sum())
    moved_rows = max(-(-n_new // TR) * TR - f // TR * TR, 0)
    moved = moved_rows * row
    hbm = 4 * moved
    if screen == "int8":
        dpad8 = max(-(-d // 64) * 64, 128)
        groups = dpad8 % 256 == 0 and dpad8 >= 512  # inner product, direct int8 screen: group means
        r0 = f // GROUP * GROUP if groups else f
        rq = max(n_new - r0, 0)
        hbm += rq * ((2 if groups else 1) * dpad * es + dpad8 + 4)
    return moved, hbm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alt-runs", type=int, default=3)
    args = ap.parse_args()
    n, d, dtype = args.n, args.d, args.dtype
    rng = np.random.default_rng(1)
    block = np.zeros(n, dtype=bool)
    block[: n // 10] = True
    last = np.zeros(n, dtype=bool)
    last[n - 1] = True
    cases = [("random_1%", rng.random(n) < 0.01), ("first_10%_block", block), ("last_row", last)]
    # the stored rows on the host, once: what reset() + add() has to start from
    ix = build(n, d, dtype, "int8")
    host = np.empty((n, d), dtype=np.float32)
    for r0 in range(0, n, 65536):
        host[r0:r0 + 65536] = ix.reconstruct_n(r0, min(65536, n - r0))
    ix.close()
    for screen in ("int8", "native"):
        for name, mask in cases:
            removed = int(mask.sum())
            ts = []
            for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
                ix = build(n, d, dtype, screen)
                t0 = time.perf_counter()
                got = ix.remove_ids(mask)
                dt = (time.perf_counter() - t0) * 1e3
                assert got == removed and ix.ntotal == n - removed
                if run == 0:  # the survivors are where they belong: the first, a middle and the last row
                    keep = np.flatnonzero(~mask)
                    for j in (0, keep.shape[0] // 2, keep.shape[0] - 1):
                        assert np.array_equal(ix.reconstruct(j), host[keep[j]]), (name, j)
                else:
                    ts.append(dt)
                ix.close()
            # (the timed call includes pack_allowed's host work, the mask -> the bitmap: ~1 ms per 1M rows)
            moved, hbm = traffic(n, d, dtype, screen, mask)
            med = float(np.median(ts))
            row = {"N": n, "d": d, "dtype": dtype, "screen": screen, "case": name, "removed": removed,
                   "remove_ms_median": round(med, 3), "remove_ms_min": round(min(ts), 3),
                   "remove_ms_all": [round(t, 3) for t in ts], "moved_bytes": moved, "predicted_hbm_bytes": hbm,
                   "implied_TBps": round(hbm / med / 1e9, 3) if med > 0 else None}
            if screen == "int8":
                survivors = np.ascontiguousarray(host[~mask]) if removed > 1 else host[: n - 1]
                ix = build(n, d, dtype, screen)
                alt = []
                for run in range(args.alt_runs + 1):
                    t0 = time.perf_counter()
                    ix.reset()
                    ix.add(survivors)
                    dt = (time.perf_counter() - t0) * 1e3
                    if run:
                        alt.append(dt)
                ix.close()
                del survivors
                row["reset_add_ms_median"] = round(float(np.median(alt)), 3)
                row["reset_add_ms_all"] = [round(t, 3) for t in alt]
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()

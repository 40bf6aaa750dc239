"""Density clusters: FlatIndex.range_degrees / range_dbscan against range_components (one self-join with the
union sink: the yardstick for what a pass costs) and against the road there was before them, host calls end to
end (each ends in a device synchronise), alternated in one process after a warm-up round.
  comp       range_components(radius): one self-join, unions
  degrees    range_degrees(radius): pass 1 alone
  dbscan2/5  range_dbscan(radius, min_samples = 2 / 5): pass 1, the core mask, pass 2, the labels
  host       range_search_rows(radius, self_mode="above"), a bincount of both ends and the recipe of
             tests/oracle_dbscan_index.py over the pair list (few and bursts only)
Corpora and radius are scripts/components_timing.py's (100k x 1536 unit rows, radius 0.95; few / bursts / big;
f32 takes the SCAN tier, bf16 the SCREEN tier).  The device results are checked against the host road's.
Reported: median / minimum / spread of the wall ms of each road, each new road as a multiple of comp, the
HIP-event split of the last dbscan5 call (vs_dbscan_last_times) and its stats.  One JSON line per case, also
appended to --out.
python scripts/dbscan_timing.py [--out profiles/dbscan_timing.jsonl] [--quick] [--reps N]"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from components_timing import RADIUS, STORES, alternate_ms, emit, plant, summary  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle_dbscan_index import dbscan_of_pairs  # noqa: E402
from photo_search_engine_amd.index import FlatIndex  # noqa: E402


def host_road(ix, min_samples):
    lims, D, I = ix.range_search_rows(RADIUS, self_mode="above")
    n = ix.ntotal
    first = np.repeat(np.arange(n, dtype=np.int64), np.diff(lims))
    return dbscan_of_pairs(np.ones((n,), dtype=bool), first, I, D, "ip", min_samples)


def same(a, b):
    return bool(all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="20k rows, fewer repetitions")
    ap.add_argument("--reps", type=int, default=0, help="repetitions per road (default 5, big 3)")
    ap.add_argument("--host-reps", type=int, default=0, help="repetitions of the host road (default: as --reps)")
    ap.add_argument("--cases", default="few,bursts,big")
    ap.add_argument("--dtypes", default="f32,bf16")
    args = ap.parse_args()
    for N, d, dtype in STORES:
        if dtype not in args.dtypes.split(","):
            continue
        if args.quick:
            N = 20_000
        for case in args.cases.split(","):
            reps = args.reps or (2 if args.quick else 3 if case == "big" else 5)
            x = O.synth_rows(O.SEED_CORPUS, 0, N, d, True, "f32")
            plant(x, case, np.random.default_rng(11))
            ix = FlatIndex(d, "ip", dtype)
            ix.add(x)
            del x
            roads = [lambda: ix.range_components(RADIUS), lambda: ix.range_degrees(RADIUS),
                     lambda: ix.range_dbscan(RADIUS, 2), lambda: ix.range_dbscan(RADIUS, 5)]
            ts, (res_comp, res_deg, res_db2, res_db5) = alternate_ms(roads, reps)
            st, tm = ix.dbscan_last_stats(), ix.dbscan_last_times()  # (of the last dbscan5 call)
            row = {"case": case, "N": N, "d": d, "dtype": dtype, "radius": RADIUS, "reps": reps,
                   "comp": summary(ts[0]), "degrees": summary(ts[1]), "dbscan2": summary(ts[2]), "dbscan5": summary(ts[3])}
            for name in ("degrees", "dbscan2", "dbscan5"):
                row[name + "_over_comp"] = round(row[name]["median_ms"] / row["comp"]["median_ms"], 3)
            row.update(edges=res_deg[1], same_edges=bool(res_deg[1] == res_comp[2] == res_db5[3]["edges"]),
                       degrees_sum_ok=bool(int(res_deg[0].sum()) == 2 * res_deg[1]),
                       counts2=res_db2[3], counts5=res_db5[3], stats5=st, times5={k: round(v, 3) for k, v in tm.items()})
            if case != "big":
                hreps = args.host_reps or reps
                th, (h2, h5) = alternate_ms([lambda: host_road(ix, 2), lambda: host_road(ix, 5)], hreps, warm=0)
                row.update(host2=summary(th[0]), host5=summary(th[1]), host_reps=hreps, same_as_host2=same(res_db2, h2),
                           same_as_host5=same(res_db5, h5), same_degrees=bool(np.array_equal(res_deg[0], h5[2])))
                row["host5_over_dbscan5"] = round(row["host5"]["median_ms"] / row["dbscan5"]["median_ms"], 3)
            else:
                m = N // 5
                row["expected"] = bool((res_deg[0][2 * N // 5:3 * N // 5] >= m - 1).all() and
                                       (res_db5[0][2 * N // 5:3 * N // 5] == 2 * N // 5).all())
                row["host"] = "not run: 2e8 pairs"
            emit(row, args.out)
            ix.close()


if __name__ == "__main__":
    main()

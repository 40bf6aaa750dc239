"""k-means over stored rows: FlatIndex.kmeans against the only clustering loop there was before it,
IVFFlatIndex.train, in one process.  Index: N synthetic rows of d (default 1M x 1536, bf16), k = 1024,
L2 assignment.  Per run FlatIndex.kmeans does --niter updates from the same seed; the library's HIP
events (vs_kmeans_last_times) split the call into assignment (gather + exact top-1 of every member),
grouping (labels, the radix sort, the host's segment list) and update (segment sums + finalize), all
divided by the passes / updates run.  The update must read every member row once, m * d * es bytes:
that over the update time is its achieved rate, to hold against the ~6.3 TB/s a streaming read
achieves.  One untimed run first; medians over --runs.  Alongside: IVFFlatIndex.train on the same rows
from host memory (every row in the training set), wall time per iteration.
One JSON line, also appended to --out.
python scripts/kmeans_timing.py [--out profiles/kmeans_timing.jsonl] [--n 1000000] [--d 1536] [--k 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from photo_search_engine_amd.index import FlatIndex, kmeans_last_times  # noqa: E402
from photo_search_engine_amd.ivf import IVFFlatIndex  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--niter", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=1, help="iterations of the IVFFlatIndex.train loop (0: skip)")
    args = ap.parse_args()
    n, d, k, dtype = args.n, args.d, args.k, args.dtype
    es = 4 if dtype == "f32" else 2
    ix = FlatIndex(d, "ip", dtype)
    ix.add_synthetic(O.SEED_CORPUS, 0, n, True)
    init = np.sort(np.random.default_rng(1234).permutation(n)[:k])
    init = np.stack([ix.reconstruct(int(i)) for i in init])  # (fetched once: not part of the timed call)
    wall, assign, group, update = [], [], [], []
    first = None
    for run in range(args.runs + 1):  # (run 0: warm-up, not recorded)
        t0 = time.perf_counter()
        res = ix.kmeans(k, niter=args.niter, init=init, metric="l2")
        dt = (time.perf_counter() - t0) * 1e3
        t = kmeans_last_times()
        assert t["updates"] == res.n_iter and t["passes"] == res.n_iter + 1
        if first is None:
            first = res
        else:  # reproducible to the bit
            assert first.centroids.tobytes() == res.centroids.tobytes() and first.labels.tobytes() == res.labels.tobytes()
        if run:
            wall.append(dt / max(res.n_iter, 1))
            assign.append(t["assign_ms"] / t["passes"])
            group.append(t["group_ms"] / max(t["updates"], 1))
            update.append(t["update_ms"] / max(t["updates"], 1))
    upd = float(np.median(update))
    row = {"N": n, "d": d, "k": k, "dtype": dtype, "niter": args.niter, "updates_run": first.n_iter,
           "wall_ms_per_iteration_median": round(float(np.median(wall)), 3),
           "assign_ms_per_pass_median": round(float(np.median(assign)), 3),
           "group_ms_per_update_median": round(float(np.median(group)), 3),
           "update_ms_per_update_median": round(upd, 3),
           "update_bytes": n * d * es, "update_TBps": round(n * d * es / upd / 1e9, 3) if upd > 0 else None,
           "largest_cluster": int(first.counts.max()), "empty_clusters": int((first.counts == 0).sum())}
    if args.train_iters > 0:
        host = np.empty((n, d), dtype=np.float32)
        for r0 in range(0, n, 65536):
            host[r0:r0 + 65536] = ix.reconstruct_n(r0, min(65536, n - r0))
        ivf = IVFFlatIndex(d, k, "l2", dtype)
        ivf.train(host[: 4 * k], niter=1, max_points_per_centroid=n)  # warm-up of the assignment path
        t0 = time.perf_counter()
        ivf.train(host, niter=args.train_iters, max_points_per_centroid=n)
        row["ivf_train_ms_per_iteration"] = round((time.perf_counter() - t0) * 1e3 / args.train_iters, 1)
        ivf.close()
    ix.close()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

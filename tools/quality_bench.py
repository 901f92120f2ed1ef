"""Times the cluster-quality kernels (csrc/quality.hip) on one GPU.

Data: cdr_points_generate's config-3 blobs (d = 16, 64 blobs) and `--steps`
device-loop Lloyd steps with k = 64, which leave the labels resident.  Then
  * silhouette of a sorted random sample of m rows for every m of --m, and
  * the Davies-Bouldin scatter pass over all n rows,
each once untimed and `--reps` times timed.  Kernel times are the library's own
HIP events around its launches (cdr_quality_timing); the call time is a host
clock around the synchronous call (gather, the host's label ranking and the
copies included).  Reports median and min..max, pair distances per second, the
share of the fp64 vector peak (both as FLOPs, 3 d + 20 per pair with the
root's 20, over 78.6 TFLOP/s, and as issue slots, 2 d + 15 fp64 instructions
per pair over 39.3e12 lane-instructions/s: the inner loop's count in the ISA),
and for the scatter pass the share of 8 TB/s HBM on n (4 d + 4) bytes.
For a CPU figure the NumPy model (tests/quality_model.py) and, where it is
installed, scikit-learn score the same m = --cpu-m rows in the same run.

    python tools/quality_bench.py [--n 100000000] [--m 16384,65536,262144] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "clustering-driven-replication-strategy_amd")
sys.path[:0] = [PKG, REPO, os.path.join(REPO, "tests")]

FP64_PEAK_FLOPS = 78.6e12   # MI355X fp64 vector, an fma counted as 2
FP64_PEAK_ISSUE = 39.3e12   # fp64 lane-instructions per second
HBM_PEAK = 8.0e12
ROOT_FLOPS, ROOT_INSTR = 20, 15  # sqrt + the add into the running sum


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--m", default="16384,65536,262144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-m", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import _cdr
    from cdr_dist import Comm, DeviceLloyd, row_fetcher, seed_sharded

    n, d, k = args.n, args.d, args.k
    ctx = _cdr.Context(0)
    ctx.generate_points(n, 0, n, d, k, args.seed)
    comm = Comm(None, None)
    C = seed_sharded(ctx, comm, 0, n, k, random_state=42)
    np.random.seed(0)
    run = DeviceLloyd(ctx, C, -1.0, row_fetcher(ctx, comm, 0, d), n, comm)
    run.advance(args.steps, chunk=args.steps, chunk_max=args.steps)
    C, _ = run.finish()
    C = np.asarray(C, dtype=np.float64)
    res = {"n": n, "d": d, "k": k, "steps": args.steps, "reps": args.reps, "silhouette": [],
           "mode": ctx.info()["mode"]}

    rng = np.random.default_rng(7)
    for m in [int(v) for v in args.m.split(",") if v]:
        m = min(m, n)
        idx = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
        kern, longest, call = [], [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            s, _, cnt = ctx.silhouette(k, idx)
            dt = (time.perf_counter() - t0) * 1e3
            tm = ctx.quality_timing()
            if rep:  # the first call is the warm-up
                kern.append(tm["pairs_ms"])
                longest.append(tm["pairs_max_launch_ms"])
                call.append(dt)
        ks = spread(kern)
        pairs = float(m) * m
        row = {"m": m, "score": float(s.mean()), "nonempty": int(np.count_nonzero(cnt)),
               "pair_launches": tm["pair_launches"], "pair_kernels_ms": ks,
               "longest_launch_ms": spread(longest), "call_ms": spread(call),
               "pairs_per_s": pairs / (ks["median"] * 1e-3),
               "fp64_flops_share": pairs * (3 * d + ROOT_FLOPS) / (ks["median"] * 1e-3)
               / FP64_PEAK_FLOPS,
               "fp64_issue_share": pairs * (2 * d + ROOT_INSTR) / (ks["median"] * 1e-3)
               / FP64_PEAK_ISSUE}
        res["silhouette"].append(row)
        print(json.dumps(row), flush=True)

    kern, call = [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        sums, counts = ctx.quality_scatter(C)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            kern.append(ctx.quality_timing()["scatter_ms"])
            call.append(dt)
    ks = spread(kern)
    res["scatter"] = {"kernels_ms": ks, "call_ms": spread(call), "bytes": n * (4 * d + 4),
                      "hbm_share": n * (4 * d + 4) / (ks["median"] * 1e-3) / HBM_PEAK,
                      "nonempty": int(np.count_nonzero(counts))}
    print(json.dumps(res["scatter"]), flush=True)

    # CPU figures on the same kind of sample
    import quality_model as qm

    m = min(args.cpu_m, n)
    idx = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    X = ctx.get_rows(idx)
    labels = ctx.labels()[idx]
    t0 = time.perf_counter()
    s_model = qm.silhouette_samples(X, labels, k)[0]
    cpu = {"m": m, "model_s": time.perf_counter() - t0, "threads": os.cpu_count()}
    try:
        from sklearn.metrics import silhouette_samples

        t0 = time.perf_counter()
        s_sk = silhouette_samples(X, labels)
        cpu["sklearn_s"] = time.perf_counter() - t0
        cpu["sklearn_vs_model"] = float(np.abs(s_sk - s_model).max())
    except ImportError:
        cpu["sklearn_s"] = None
    t0 = time.perf_counter()
    s_dev = ctx.silhouette(k, idx)[0]
    cpu["device_call_s"] = time.perf_counter() - t0
    cpu["device_vs_model"] = float(np.abs(s_dev - s_model).max())
    res["cpu"] = cpu
    print(json.dumps(cpu), flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

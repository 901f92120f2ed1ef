"""Times the global feature medians (csrc/medians.hip gm_hist32 / gm_hist64,
Context.medians_global) on one GPU, against the two routes there were before.

Points: cdr_points_generate's blobs (F32X; config 3 = 100M x 16, config 5 =
50M x 64), or with --f64 the F64 leg's points as tools/f64_time.py builds them
(blobs min-max normalised on the host, 10M x 5).  Per size:

  1. the new call, once untimed and --reps times timed: a host clock around the
     synchronous call, and the library's own HIP events around its histogram
     launches (cdr_medians_global_timing).  The pass time is set against the
     n d (4 | 8) bytes a pass reads.
  2. the only device route without it: one Lloyd step with a single centroid,
     then medians_by_label(1) (a grouped copy of every row, then mg_hist on one
     workgroup per 64-feature chunk).  It is slow enough that --route2-rows can
     give it (and the new call next to it) fewer rows of the same generator;
     one workgroup streams the rows, so its time is linear in n.
  3. np.median(X, axis=0) on the host over --host-rows rows fetched back (a
     sample when that is less than n: the JSON says so).

--degenerate-rows N times one pass-set over an N x 16 table of one constant
(every wave's lanes agree on the digit in every pass) beside one of uniform
random values on the 2^-24 grid.

    python tools/global_medians_bench.py --name config3 --n 100000000 --d 16 --out FILE
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "clustering-driven-replication-strategy_amd")
sys.path[:0] = [PKG, REPO]


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def build(_cdr, n, d, f64, seed):
    ctx = _cdr.Context(0)
    ctx.generate_points(n, 0, n, d, 16, seed)
    if not f64:
        return ctx
    X = ctx.get_rows(np.arange(n, dtype=np.int64))
    mn, mx = X.min(axis=0), X.max(axis=0)
    X = (X - mn) / (mx - mn)
    ctx.load_points(X)
    assert ctx.info()["mode"] == _cdr.MODE_F64
    return ctx


def time_new(ctx, reps):
    inf = ctx.info()
    n, d = inf["n"], inf["d"]
    size = 4 if inf["mode"] == 1 else 8
    call, kern, longest, each = [], [], [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        med = ctx.medians_global()
        dt = (time.perf_counter() - t0) * 1e3
        tm = ctx.medians_global_timing()
        if rep:  # the first call is the warm-up
            call.append(dt)
            kern.append(tm["hist_ms"])
            longest.append(tm["hist_max_ms"])
            each.append(tm["pass_ms"])
    per_pass = spread(kern)["median"] / tm["passes"]
    return {"n": n, "d": d, "passes": tm["passes"], "call_ms": spread(call),
            "hist_kernels_ms": spread(kern), "longest_pass_ms": spread(longest),
            "pass_ms": per_pass,
            "each_pass_ms": [float(v) for v in np.median(np.array(each), axis=0)],
            "pass_bytes": n * d * size,
            "pass_bytes_per_s": n * d * size / (per_pass * 1e-3)}, med


def time_route2(ctx):
    inf = ctx.info()
    d = inf["d"]
    C = ctx.get_rows(np.array([0], dtype=np.int64)).reshape(1, d)
    t0 = time.perf_counter()
    if inf["mode"] == 1:
        ctx.lloyd_step(C)
    else:
        ctx.lloyd_step_f64(C)
    step = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    med = ctx.medians_by_label(1)[0]
    return {"n": inf["n"], "d": d, "lloyd_step_ms": step,
            "medians_by_label_ms": (time.perf_counter() - t0) * 1e3}, med


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="run")
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route2-rows", type=int, default=-1, help="-1: all n rows; 0: skip")
    ap.add_argument("--host-rows", type=int, default=4_000_000)
    ap.add_argument("--degenerate-rows", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import _cdr

    res = {"name": args.name, "f64": args.f64, "reps": args.reps}
    ctx = build(_cdr, args.n, args.d, args.f64, args.seed)
    res["mode"] = ctx.info()["mode"]
    res["new"], med = time_new(ctx, args.reps)
    print(json.dumps(res["new"]), flush=True)

    # 3. the host, on the first host_rows rows
    m = min(args.host_rows, args.n)
    X = ctx.get_rows(np.arange(m, dtype=np.int64))
    t0 = time.perf_counter()
    hmed = np.median(X, axis=0)
    res["host"] = {"rows": m, "is_sample": m < args.n, "np_median_s": time.perf_counter() - t0,
                   "threads": os.cpu_count()}
    if m == args.n:
        res["host"]["equal"] = bool(np.array_equal(hmed, med))
    del X
    print(json.dumps(res["host"]), flush=True)

    # 2. route 2 on the same context, or on fewer rows of the same generator
    r2 = args.n if args.route2_rows < 0 else args.route2_rows
    if r2:
        if r2 != args.n:
            ctx.close()
            ctx = build(_cdr, r2, args.d, args.f64, args.seed)
            res["new_at_route2_rows"], med = time_new(ctx, args.reps)
        new = res.get("new_at_route2_rows", res["new"])
        res["route2"], med2 = time_route2(ctx)
        res["route2"]["equal"] = bool(np.array_equal(med2, med))
        res["route2"]["ratio_to_new_call"] = (res["route2"]["medians_by_label_ms"]
                                              / new["call_ms"]["median"])
        print(json.dumps(res["route2"]), flush=True)
    ctx.close()

    if args.degenerate_rows:
        nn = args.degenerate_rows
        ctx = _cdr.Context(0)
        rng = np.random.default_rng(1)
        tables = {"constant": np.full((nn, 16), 0.375),
                  "random": np.floor(rng.random((nn, 16)) * 2.0 ** 24) * 2.0 ** -24}
        res["degenerate"] = {}
        for key, X in tables.items():
            ctx.load_points(X)
            assert ctx.info()["mode"] == 1
            row, _ = time_new(ctx, args.reps)
            res["degenerate"][key] = row
            print(key, json.dumps(row), flush=True)
        ctx.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        allres = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                allres = json.load(fh)
        allres[args.name] = res
        with open(args.out, "w") as fh:
            json.dump(allres, fh, indent=1)


if __name__ == "__main__":
    main()

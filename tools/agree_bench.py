"""Times the contingency table of two clusterings on one GPU.

Data: cdr_points_generate's config-3 blobs (d = 16, 64 blobs), for every row
count of --rows and every k of --ks two k-means runs (seeds 42 and 43, --steps
Lloyd steps each) on the resident points.  The first run's labels are kept on
the device (cdr_agree_keep), the second run's stay resident.  Per (n, k), with
and without sizes (random below 2^40 bytes):

  file    the table of the resident against the kept labels, in row order;
  sorted  the same rows sorted by the resident cluster (explicit labels: the
          upload is in `upload_ms`, not in the kernel time): whole waves in one
          cell, the same-address worst case;
  host    the route without the kernel: two ctx.labels() read-backs of n int64
          and np.bincount(a * k + b).

Each is run once untimed and --reps times timed.  Reports median and min..max
of the kernel time (HIP events, cdr_agree_timing) and of the call on the host
clock, the bytes the kernel reads over its time against the 8 TB/s HBM peak,
and for the global form the integer atomics per second.  The device table is
compared with the host route's once per (n, k).  Results are written after
every (n, k).

    python tools/agree_bench.py [--rows 10000000,100000000] [--ks 64,1024]
                                [--out profiles/agree_bench.json]
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

HBM_PEAK = 8.0e12  # bytes / s


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def cluster(ctx, n, d, k, seed, steps):
    from cdr_dist import Comm, DeviceLloyd, row_fetcher, seed_sharded

    comm = Comm(None, None)
    C = seed_sharded(ctx, comm, 0, n, k, random_state=seed)
    np.random.seed(0)
    run = DeviceLloyd(ctx, C, -1.0, row_fetcher(ctx, comm, 0, d), n, comm)
    run.advance(steps, chunk=steps, chunk_max=steps)
    run.finish()


def timed(ctx, reps, fn):
    kern, call, up, back = [], [], [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        t = ctx.agree_timing()
        if rep:  # the first call is the warm-up
            kern.append(float(t[1]))
            call.append(dt)
            up.append(float(t[0]))
            back.append(float(t[2]))
    return out, {"kernel_ms": spread(kern), "call_ms": spread(call), "upload_ms": spread(up),
                 "copy_back_ms": spread(back)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000000,100000000")
    ap.add_argument("--ks", default="64,1024")
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "agree_bench.json"))
    args = ap.parse_args()

    import _cdr

    res = {"d": args.d, "blobs": args.blobs, "steps": args.steps, "reps": args.reps, "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ctx = _cdr.Context(0)
    for n in [int(v) for v in args.rows.split(",") if v]:
        ctx.generate_points(n, 0, n, args.d, args.blobs, args.seed)
        sizes = np.random.default_rng(n).integers(0, 2 ** 40, n).astype(np.int64)
        for k in [int(v) for v in args.ks.split(",") if v]:
            try:
                cluster(ctx, n, args.d, k, 42, args.steps)
                ctx.agree_keep()
                kept = ctx.labels()
                cluster(ctx, n, args.d, k, 43, args.steps)
            except (NotImplementedError, ValueError) as e:  # a shape k-means does not take
                res["runs"].append({"n": n, "k": k, "error": str(e)})
                print(json.dumps(res["runs"][-1]), flush=True)
                continue

            # the host route: both label arrays read back, one bincount
            host = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                a = ctx.labels()
                b = ctx.labels()  # (the second run's read-back stands in for the first's: same bytes)
                table = np.bincount(a * k + b, minlength=k * k).reshape(k, k)
                if rep:
                    host.append((time.perf_counter() - t0) * 1e3)
            want = np.bincount(a * k + kept, minlength=k * k).reshape(k, k)
            order = np.argsort(a, kind="stable")
            a_sorted, b_sorted = a[order], kept[order]
            s_sorted = sizes[order]
            del order, table, b

            row = {"n": n, "k": k, "host_route_ms": spread(host), "cases": {}}
            same = True
            for with_sizes in (False, True):
                per_row = 16 if with_sizes else 8
                for order_name, fn in (
                        ("file", lambda: ctx.agree_table(k, k, None, None,
                                                         sizes if with_sizes else None)),
                        ("sorted", lambda: ctx.agree_table(k, k, a_sorted, b_sorted,
                                                           s_sorted if with_sizes else None))):
                    out, t = timed(ctx, args.reps, fn)
                    counts = out[0] if with_sizes else out
                    same = same and bool(np.array_equal(counts, want))
                    info = ctx.agree_info()
                    sec = t["kernel_ms"]["median"] * 1e-3
                    t.update(form=info["form"], workgroups=info["workgroups"],
                             read_bytes=n * per_row, read_bytes_per_s=n * per_row / sec,
                             hbm_peak_share=n * per_row / sec / HBM_PEAK)
                    if info["form"] == 1:
                        # an upper bound of the adds: 1 count and 2 size halves per row (a
                        # group of 64 rows in one cell adds once)
                        t["atomics_per_s"] = n * (3 if with_sizes else 1) / sec
                    row["cases"][f"{order_name}{'_sizes' if with_sizes else ''}"] = t
            row["same_as_host"] = same
            row["host_over_device_call"] = (row["host_route_ms"]["median"]
                                            / row["cases"]["file"]["call_ms"]["median"])
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
            del a, kept, a_sorted, b_sorted, s_sorted
    ctx.close()


if __name__ == "__main__":
    main()

"""Times the read of the features CSV: the reference's
``pd.read_csv(path)[CLUSTERING_FEATURES].values`` (src/main.py:75-81) against
``features_csv.read_features`` (csrc/csvin.hip) on one GPU.

The file: feature-like rows (tests/csv_cases.feature_table) with paths of about
30 bytes, written by the project's own writer (write_spark_csv_device), for
every row count of --rows.  Each reader runs once untimed and --reps times
timed on the file in the page cache.  Per device run: the whole call (host
clock around read_features: the mmap, the header, the library calls, X copied
out) and the library's HIP-event split (cdr_csv_read_timing: upload, record
index, parse kernel, finish).  Reports median and min..max, the parse
kernel's file bytes per second, and the ratio of the whole calls.  The values
are compared by bits once per file.

    python tools/csv_read_bench.py [--rows 1000000,4000000] [--out profiles/csv_read_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "clustering-driven-replication-strategy_amd")
sys.path[:0] = [PKG, REPO, os.path.join(REPO, "tests")]


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,4000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temp dir)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csv_read_bench.json"))
    args = ap.parse_args()

    import pandas as pd

    import _cdr
    import compute_features as cf
    import csv_cases as cc
    from features_csv import CLUSTERING_FEATURES, read_features

    base = tempfile.mkdtemp(prefix="csv_read_bench_", dir=args.dir)
    res = {"reps": args.reps, "columns": CLUSTERING_FEATURES, "runs": []}
    ctx = _cdr.Context(0)
    try:
        for n in [int(v) for v in args.rows.split(",") if v]:
            table, paths = cc.feature_table(n), cc.feature_paths(n)
            part = cf.write_spark_csv_device(os.path.join(base, "f"), paths, table, ctx=ctx)
            del table, paths
            size = os.path.getsize(part)
            host, want = [], None
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                want = pd.read_csv(part)[CLUSTERING_FEATURES].values
                if rep:  # the first run is the warm-up
                    host.append(time.perf_counter() - t0)
            whole, split, info, X = [], [], {}, None
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                X = read_features(part, ctx=ctx, info=info)
                dt = time.perf_counter() - t0
                if rep:
                    whole.append(dt)
                    split.append([info["upload_ms"], info["index_ms"], info["parse_ms"],
                                  info["finish_ms"]])
            same = bool((X.view(np.uint64) == want.astype(np.float64).view(np.uint64)).all())
            split = np.array(split)
            h, w = spread(host), spread(whole)
            parse = spread(split[:, 2].tolist())
            row = {"rows": n, "bytes": size, "same_bits": same,
                   "deferred_rows": info["deferred_rows"],
                   "whole_file_fallback": info["whole_file_fallback"],
                   "pandas_s": h, "read_features_s": w,
                   "upload_ms": spread(split[:, 0].tolist()),
                   "index_ms": spread(split[:, 1].tolist()), "parse_ms": parse,
                   "finish_ms": spread(split[:, 3].tolist()),
                   "parse_file_bytes_per_s": size / (parse["median"] * 1e-3),
                   "index_file_bytes_per_s": size / (spread(split[:, 1].tolist())["median"] * 1e-3),
                   "ratio_to_pandas": h["median"] / w["median"]}
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
            del X, want
            shutil.rmtree(os.path.join(base, "f"), ignore_errors=True)
        ctx.close()
    finally:
        shutil.rmtree(base, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

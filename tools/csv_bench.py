"""Times the features CSV writers: the host's write_spark_csv against
write_spark_csv_device (csrc/csvout.hip) on one GPU.

Table: feature-like rows (tests/csv_cases.feature_table: counts, ages with a
millisecond fraction, ratios of counts, min-max norms) with paths of about 30
bytes.  The host writer formats --host-rows rows (20 000), the device writer
every row count of --rows (1M and 16M), each once untimed and --reps times
timed, into a fresh directory under --dir.  Per device run: the whole call
(host clock around write_spark_csv_device: packing the paths, the library
calls, the splice, the file write), the time inside Context.csv_format, and the
library's own HIP-event split summed over the chunks (cdr_csv_timing: cell
kernel, scan + emit kernels, copies).  Reports median and min..max and the
rows/s ratio of the device writer's whole call to the host writer.

    python tools/csv_bench.py [--rows 1000000,16000000] [--out profiles/csv_bench.json]
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


class Timed:
    """The context with a clock around csv_format and its event times summed."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.reset()

    def reset(self):
        self.call_s, self.ms, self.calls = 0.0, np.zeros(3), 0

    def csv_format(self, table, paths, long_cols=()):
        t0 = time.perf_counter()
        out = self.ctx.csv_format(table, paths, long_cols)
        self.call_s += time.perf_counter() - t0
        self.ms += self.ctx.csv_timing()
        self.calls += 1
        return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,16000000")
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temp dir)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csv_bench.json"))
    args = ap.parse_args()

    import _cdr
    import compute_features as cf
    import csv_cases as cc

    base = tempfile.mkdtemp(prefix="csv_bench_", dir=args.dir)
    res = {"reps": args.reps, "chunk_rows": cf.CSV_CHUNK_ROWS, "device": []}
    try:
        n = args.host_rows
        table, paths = cc.feature_table(n), cc.feature_paths(n)
        times = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            part = cf.write_spark_csv(os.path.join(base, "host"), paths, table)
            if rep:  # the first run is the warm-up
                times.append(time.perf_counter() - t0)
        host = {"rows": n, "bytes_per_row": (os.path.getsize(part) - 120) / n, "s": spread(times),
                "rows_per_s": n / spread(times)["median"]}
        res["host"] = host
        print(json.dumps(host), flush=True)

        ctx = _cdr.Context(0)
        timed = Timed(ctx)
        for n in [int(v) for v in args.rows.split(",") if v]:
            table, paths = cc.feature_table(n), cc.feature_paths(n)
            whole, inside, split = [], [], []
            for rep in range(args.reps + 1):
                timed.reset()
                t0 = time.perf_counter()
                part = cf.write_spark_csv_device(os.path.join(base, "dev"), paths, table, ctx=timed)
                dt = time.perf_counter() - t0
                if rep:
                    whole.append(dt)
                    inside.append(timed.call_s)
                    split.append(timed.ms.copy())
            split = np.array(split)
            w = spread(whole)
            row = {"rows": n, "bytes": os.path.getsize(part), "calls": timed.calls,
                   "deferred": timed.last_csv["deferred"], "whole_s": w,
                   "csv_format_s": spread(inside),
                   "cell_kernel_ms": spread(split[:, 0].tolist()),
                   "scan_emit_ms": spread(split[:, 1].tolist()),
                   "copies_ms": spread(split[:, 2].tolist()),
                   "rows_per_s": n / w["median"],
                   "ratio_to_host": n / w["median"] / host["rows_per_s"]}
            res["device"].append(row)
            print(json.dumps(row), flush=True)
            del table, paths
        ctx.close()
    finally:
        shutil.rmtree(base, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

"""Times the replica placement on one GPU.

Data: the device access simulator's log at the config-4 share (bench.py's
FEATURES_CFG files, 600 s, --clients datanodes, ~125M events), then the same
events with the clients and primaries spread over --wide-nodes nodes (loaded
with cdr_features_load_events).  Labels are random in [0, 4), factors 3, 2, 1,
2, sizes random below 2^40 bytes.  Per data set:

  groupby  the group-by's own step under cdr_profile_*: partition ms and bucket
           kernel ms (that kernel reads the same payload, 4 B per event: the
           yardstick of the placement kernel);
  reused   place_replicas with the resident partition reused;
  built    place_replicas after the events were loaded anew (partition built);
  global   the same call with CDR_PLACE_GLOBAL=1;
  host     the only route without the kernels: features_events_read and
           placement_host on the CPU (once).

Each device case runs once untimed and --reps times timed (the built case
--reps-built times: every rep uploads the log again).  Reports the median and
min..max of cdr_place_timing's four parts and of the call on the host clock,
the payload bytes over the kernel time against the 8 TB/s HBM peak, and for
the global form the integer atomics per second.  The device result is compared
with the host route's once per data set.  One JSON line per data set.

    python tools/place_bench.py [--events 125000000] [--out profiles/place_bench.json]
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
K, FACTORS, R = 4, [3, 2, 1, 2], 3


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def timed(ctx, reps, fn, before=None):
    parts, call = [], []
    out = None
    for rep in range(reps + 1):
        if before is not None:
            before()
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if rep:  # the first call is the warm-up
            parts.append(ctx.place_timing().tolist())
            call.append(dt)
    names = ("partition_ms", "upload_ms", "kernel_ms", "copy_back_ms")
    res = {nm: spread([p[i] for p in parts]) for i, nm in enumerate(names)}
    res["call_ms"] = spread(call)
    return out, res


def same(a, b):
    return bool(all(np.array_equal(a[key], b[key]) for key in ("nodes", "per_file", "cluster_sums",
                                                               "node_replicas"))
                and a["node_bytes"] == b["node_bytes"])


def measure(ctx, name, n_nodes, args, events):
    from replica_placement import placement_host

    f, op, cl, ts, prim = events
    ne, nf = f.size, prim.size
    rng = np.random.default_rng(nf)
    labels = rng.integers(0, K, nf).astype(np.int64)
    sizes = rng.integers(0, 2 ** 40, nf).astype(np.int64)
    row = {"data": name, "events": int(ne), "files": int(nf), "n_nodes": n_nodes, "k": K,
           "factors": FACTORS, "R": R, "reps": args.reps}

    def place():
        return ctx.place_replicas(n_nodes, K, FACTORS, R, labels=labels, sizes=sizes)

    # the group-by's own step: partition and bucket kernel
    ctx.features_aggregate_resident(to_host=False)
    ctx.profile_reset(True)
    for _ in range(args.reps):
        ctx.features_aggregate_resident(to_host=False)
    p = ctx.profile_read()
    ctx.profile_reset(False)
    steps = max(p["steps"], 1)
    gb = ctx.features_groupby_info()
    row["groupby"] = {"partition_ms": p["screen_ms"] / steps,
                      "bucket_kernel_ms": (p["step_ms"] - p["screen_ms"]) / steps, "info": gb}

    dev, row["reused"] = timed(ctx, args.reps, place)
    info = ctx.place_info()
    row["reused"]["info"] = info
    pay = ne * info["payload_bytes"]
    sec = row["reused"]["kernel_ms"]["median"] * 1e-3
    row["reused"].update(payload_bytes=pay, payload_bytes_per_s=pay / sec,
                         hbm_peak_share=pay / sec / HBM_PEAK)
    row["kernel_over_groupby_bucket_kernel"] = (row["reused"]["kernel_ms"]["median"]
                                                / row["groupby"]["bucket_kernel_ms"])

    _, row["built"] = timed(ctx, args.reps_built, place,
                            before=lambda: ctx.features_load_events(f, op, cl, ts, prim))
    row["built"]["info"] = ctx.place_info()

    os.environ["CDR_PLACE_GLOBAL"] = "1"
    try:
        glob, row["global"] = timed(ctx, args.reps, place)
        row["global"]["info"] = ctx.place_info()
    finally:
        del os.environ["CDR_PLACE_GLOBAL"]
    row["global"]["atomics_per_s"] = ne / (row["global"]["kernel_ms"]["median"] * 1e-3)
    row["bucket_over_global_kernel"] = (row["reused"]["kernel_ms"]["median"]
                                        / row["global"]["kernel_ms"]["median"])

    t0 = time.perf_counter()
    hf, _, hc, _, hp = ctx.features_events_read()
    t1 = time.perf_counter()
    host = placement_host(hf, hc, hp, n_nodes, np.asarray(FACTORS)[labels], R, sizes=sizes,
                          labels=labels, k=K)
    t2 = time.perf_counter()
    row["host"] = {"events_read_ms": (t1 - t0) * 1e3, "placement_host_ms": (t2 - t1) * 1e3,
                   "route_ms": (t2 - t0) * 1e3}
    row["same_as_host"] = same(dev, host) and same(glob, host)
    row["host_over_device_call"] = row["host"]["route_ms"] / row["reused"]["call_ms"]["median"]
    tot = int(host["per_file"][:, 0].sum())
    row["locality_before"] = float(host["per_file"][:, 1].sum() / max(tot, 1))
    row["locality_after"] = float(host["per_file"][:, 2].sum() / max(tot, 1))
    return row


def main() -> None:
    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=float, default=bench.FEATURES_CFG[0] * bench.EVENTS_PER_FILE)
    ap.add_argument("--clients", type=int, default=4)
    ap.add_argument("--wide-nodes", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-built", type=int, default=3)  # (odd: spread's median is a middle value)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "place_bench.json"))
    args = ap.parse_args()

    import _cdr

    nf = max(1, int(args.events / bench.EVENTS_PER_FILE))
    ctx = _cdr.Context(0)
    ctx.features_simulate(nf, bench.FEATURES_CFG[1], args.clients, seed=args.seed)
    ev = ctx.features_events_read()
    rows = [measure(ctx, "simulated", args.clients, args, ev)]
    print(json.dumps(rows[-1]), flush=True)
    # the same events over more nodes: node = client * s + (file + event) % s
    s = max(1, args.wide_nodes // args.clients)
    f, op, cl, ts, prim = ev
    e = np.arange(f.size, dtype=np.int64)
    cl = np.where(cl >= 0, cl * s + (f + e) % s, cl).astype(np.int32)
    prim = np.where(prim >= 0, prim * s + np.arange(prim.size) % s, prim).astype(np.int32)
    del e
    ctx.features_load_events(f, op, cl, ts, prim)
    rows.append(measure(ctx, "wide", s * args.clients, args, (f, op, cl, ts, prim)))
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

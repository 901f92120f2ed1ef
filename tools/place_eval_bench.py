"""Times the evaluation of a given placement on one GPU.

Data: as tools/place_bench.py: the device access simulator's
log at the config-4 share (bench.py's FEATURES_CFG files, 600 s, --clients
datanodes, ~125M events), then the same events with the clients and primaries
spread over --wide-nodes nodes.  Labels are random in [0, 4); the placement
that is judged is the device's own (place_replicas, factors 3, 2, 1, 2, R = 3).
Per data set:

  sums      place_evaluate without the per-file table;
  per_file  the same call with it (one or two more integer atomics per event),
            alternating with the above;
  host      the only route without the kernels: features_events_read and
            evaluate_host on the CPU (once).

Each device case runs once untimed and --reps times timed.  Reports the median
and min..max of cdr_place_evaluate_timing's four parts and of the call on the
host clock, and the event kernel's bytes per event over its time against the
8 TB/s HBM peak: 9 B streamed per event (ev_file, ev_client, ev_op) and 16 B
gathered (the file's record; 744 000 x 16 B = 12 MB, served by the caches,
one line per event).  The
device result is compared with the host route's once per data set; identity
I1 of DESIGN §13.1 is checked against the placement's own sums.  One JSON line
per data set; --place-bench adds place_bucket's §13.3 figures for scale.

    python tools/place_eval_bench.py [--events 125000000] [--out profiles/place_eval_bench.json]
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
STREAM_BYTES, GATHER_BYTES = 9, 16
PARTS = ("upload_ms", "file_pass_ms", "event_kernel_ms", "copy_back_ms")


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def timed(ctx, reps, cases):
    """``cases``: name -> fn.  One warm-up round, then ``reps`` rounds that
    run every case in turn (so the forms alternate)."""
    parts = {nm: [] for nm in cases}
    call = {nm: [] for nm in cases}
    out, info = {}, {}
    for rep in range(reps + 1):
        for nm, fn in cases.items():
            t0 = time.perf_counter()
            out[nm] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep:  # the first round is the warm-up
                parts[nm].append(ctx.place_evaluate_timing().tolist())
                call[nm].append(dt)
            info[nm] = ctx.place_evaluate_info()
    res = {}
    for nm in cases:
        res[nm] = {p: spread([row[i] for row in parts[nm]]) for i, p in enumerate(PARTS)}
        res[nm]["call_ms"] = spread(call[nm])
        res[nm]["info"] = info[nm]
    return out, res


def measure(ctx, name, n_nodes, args):
    from replica_placement import evaluate_host

    ne, nf = ctx._ev
    rng = np.random.default_rng(nf)
    labels = rng.integers(0, K, nf).astype(np.int64)
    placed = ctx.place_replicas(n_nodes, K, FACTORS, R, labels=labels)
    nodes = placed["nodes"]
    row = {"data": name, "events": int(ne), "files": int(nf), "n_nodes": n_nodes, "k": K,
           "factors": FACTORS, "R": R, "reps": args.reps}

    def ev(per_file):
        return lambda: ctx.place_evaluate(n_nodes, nodes, K, labels=labels, per_file=per_file)

    out, res = timed(ctx, args.reps, {"sums": ev(False), "per_file": ev(True)})
    row.update(res)
    for nm in res:
        sec = res[nm]["event_kernel_ms"]["median"] * 1e-3
        res[nm].update(events_per_s=ne / sec,
                       stream_bytes_per_s=ne * STREAM_BYTES / sec,
                       stream_share_of_hbm_peak=ne * STREAM_BYTES / sec / HBM_PEAK,
                       stream_and_gather_bytes_per_s=ne * (STREAM_BYTES + GATHER_BYTES) / sec)
    row["bytes_per_event"] = {"streamed": STREAM_BYTES, "gathered": GATHER_BYTES}
    pf = out["per_file"]["per_file"]
    row["per_file_atomics_per_s"] = int(pf.sum()) / (
        res["per_file"]["event_kernel_ms"]["median"] * 1e-3)

    t0 = time.perf_counter()
    hf, hop, hc, _, _ = ctx.features_events_read()
    t1 = time.perf_counter()
    host = evaluate_host(hf, hop, hc, nodes, n_nodes, labels=labels, k=K)
    t2 = time.perf_counter()
    del hf, hop, hc
    row["host"] = {"events_read_ms": (t1 - t0) * 1e3, "evaluate_host_ms": (t2 - t1) * 1e3,
                   "route_ms": (t2 - t0) * 1e3}
    row["same_as_host"] = bool(
        all(np.array_equal(out[nm]["cluster_sums"], host["cluster_sums"])
            and np.array_equal(out[nm]["node_sums"], host["node_sums"]) for nm in out)
        and np.array_equal(pf, host["per_file"]))
    row["identity_I1"] = bool(
        np.array_equal(pf, placed["per_file"][:, [0, 2]])
        and np.array_equal(host["cluster_sums"][:, 0:2], placed["cluster_sums"][:, [0, 2]])
        and np.array_equal(host["node_sums"][:, 4], placed["node_replicas"]))
    row["host_over_device_call"] = row["host"]["route_ms"] / res["sums"]["call_ms"]["median"]
    row["host_over_device_call_per_file"] = (row["host"]["route_ms"]
                                             / res["per_file"]["call_ms"]["median"])
    cs = host["cluster_sums"].sum(axis=0)
    row["locality"] = float(cs[1] / max(cs[0], 1))
    row["read_locality"] = float(cs[3] / max(cs[2], 1))
    row["write_amplification"] = float(cs[5] / max(cs[4], 1))
    row["reads_served"] = host["node_sums"][:, 2].tolist()
    return row


def main() -> None:
    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=float, default=bench.FEATURES_CFG[0] * bench.EVENTS_PER_FILE)
    ap.add_argument("--clients", type=int, default=4)
    ap.add_argument("--wide-nodes", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--place-bench", default=os.path.join(REPO, "profiles", "place_bench.json"),
                    help="tools/place_bench.py's output: its place_bucket figures, for scale")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "place_eval_bench.json"))
    args = ap.parse_args()

    import _cdr

    scale = {}
    if os.path.exists(args.place_bench):
        with open(args.place_bench) as fh:
            for line in fh:
                r = json.loads(line)
                scale[r["data"]] = {"events": r["events"],
                                    "place_bucket_kernel_ms": r["reused"]["kernel_ms"],
                                    "place_bucket_call_ms": r["reused"]["call_ms"],
                                    "global_form_kernel_ms": r["global"]["kernel_ms"]}

    nf = max(1, int(args.events / bench.EVENTS_PER_FILE))
    ctx = _cdr.Context(0)
    ctx.features_simulate(nf, bench.FEATURES_CFG[1], args.clients, seed=args.seed)
    rows = [measure(ctx, "simulated", args.clients, args)]
    rows[-1]["place_bench"] = scale.get("simulated")
    print(json.dumps(rows[-1]), flush=True)
    # the same events over more nodes: node = client * s + (file + event) % s
    s = max(1, args.wide_nodes // args.clients)
    f, op, cl, ts, prim = ctx.features_events_read()
    e = np.arange(f.size, dtype=np.int64)
    cl = np.where(cl >= 0, cl * s + (f + e) % s, cl).astype(np.int32)
    prim = np.where(prim >= 0, prim * s + np.arange(prim.size) % s, prim).astype(np.int32)
    del e
    ctx.features_load_events(f, op, cl, ts, prim)
    del f, op, cl, ts
    rows.append(measure(ctx, "wide", s * args.clients, args))
    rows[-1]["place_bench"] = scale.get("wide")
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

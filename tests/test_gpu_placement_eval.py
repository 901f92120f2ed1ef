"""The evaluation of a given placement on the device (csrc/place_eval.hip,
replica_placement.py) equals evaluate_host's integers: node counts, row widths,
cluster counts, the event kernel with and without the per-file table, every
chunk boundary of the event stream, counter widths, contention, the identities
with place_replicas and the group-by, every loader, labels, errors, untouched
state, and end to end on the golden pipeline."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_placement import _golden_inputs, events, load

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")
GOLDEN_CSV = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
T0 = 1_700_000_000_000_000
PLAIN, PER_FILE = 0, 1     # cdr_place_evaluate_info: the event kernel's two forms
# csrc/place_eval.hip: a lane reads 8 events per sweep, a wave 512, a workgroup
# of four waves 2048; the grid is ceil(events / 2048) workgroups up to what the
# device holds at once (one grid sweep = workgroups * 2048 events)
WAVE_CHUNK, WG_CHUNK = 512, 2048


def placement(rng, nf, n_nodes, R):
    """Rows with duplicates, -1 in front, in the middle and all -1."""
    nodes = rng.integers(-1, n_nodes, (nf, R)).astype(np.int32)
    nodes[rng.random(nf) < 0.1] = -1
    return nodes


def compare(ctx, f, op, cl, nodes, n_nodes, k, labels, dev_labels="host", **want):
    """place_evaluate over the resident events, with and without the per-file
    table, against the definition."""
    from replica_placement import evaluate_host

    exp = evaluate_host(f, op, cl, nodes, n_nodes, labels=labels, k=k)
    for per_file in (True, False):
        got = ctx.place_evaluate(n_nodes, nodes, k, labels=labels if dev_labels == "host" else None,
                                 per_file=per_file)
        info = ctx.place_evaluate_info()
        np.testing.assert_array_equal(got["cluster_sums"], exp["cluster_sums"])
        np.testing.assert_array_equal(got["node_sums"], exp["node_sums"])
        if per_file:
            np.testing.assert_array_equal(got["per_file"], exp["per_file"])
        else:
            assert got["per_file"] is None
        assert info["form"] == (PER_FILE if per_file else PLAIN)
        assert info["workgroup_events"] == WG_CHUNK
        for key, v in want.items():
            assert info[key] == v, (key, info)
    return got, exp, info


@pytest.mark.parametrize("n_nodes", [1, 2, 3, 4, 5, 63, 64])
def test_node_counts_and_row_widths(ctx, n_nodes):
    rng = np.random.default_rng(n_nodes)
    f, op, cl, ts, prim = events(rng, 60_000, 700, n_nodes)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, 4, 700)
    for R in (1, 3, 8):
        compare(ctx, f, op, cl, placement(rng, 700, n_nodes, R), n_nodes, 4, labels,
                workgroups=-(-60_000 // WG_CHUNK))


@pytest.mark.parametrize("k", [1, 4, 9, 1024])
def test_cluster_counts(ctx, k):
    rng = np.random.default_rng(k)
    f, op, cl, ts, prim = events(rng, 60_000, 700, 5)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, k, 700)
    labels[:2] = [0, k - 1]
    compare(ctx, f, op, cl, placement(rng, 700, 5, 3), 5, k, labels)


def test_event_kinds(ctx):
    """Paths not in the manifest, clients -3, -1, n_nodes and 200, ops 0, 1, 2."""
    rng = np.random.default_rng(7)
    f, op, cl, ts, prim = events(rng, 80_000, 300, 4, bad=0.2)
    f[:100] = 300 + np.arange(100) % 3        # past the files (the loader keeps them)
    cl = rng.choice(np.array([-3, -1, 0, 1, 2, 3, 4, 200], dtype=np.int32), f.size)
    load(ctx, f, op, cl, ts, prim)
    _, exp, _ = compare(ctx, f, op, cl, placement(rng, 300, 4, 3), 4, 4, rng.integers(0, 4, 300))
    assert exp["unserved_reads"] > 0 and 0 < exp["cluster_sums"][:, 1].sum() < (f >= 0).sum()
    assert set(np.unique(op)) == {0, 1, 2}


@pytest.mark.parametrize("ne", [1, WAVE_CHUNK - 1, WAVE_CHUNK, WAVE_CHUNK + 1, WG_CHUNK - 1,
                                WG_CHUNK, WG_CHUNK + 1])
def test_wave_and_workgroup_chunks(ctx, ne):
    rng = np.random.default_rng(ne)
    f, op, cl, ts, prim = events(rng, ne, 70, 3, bad=0.0)
    load(ctx, f, op, cl, ts, prim)
    got, exp, _ = compare(ctx, f, op, cl, placement(rng, 70, 3, 2), 3, 2, rng.integers(0, 2, 70),
                          workgroups=-(-ne // WG_CHUNK))
    assert exp["cluster_sums"][:, 0].sum() == ne        # the last event counts, none past it


def test_one_grid_sweep(ctx):
    """k = 1024 takes 50 KiB of LDS per workgroup, so few workgroups are
    resident and one sweep of the whole grid is one or two million events: one
    event fewer, exactly that, one more (the first workgroup's second sweep)."""
    rng = np.random.default_rng(31)
    nf, n_nodes, k = 1000, 4, 1024
    f, op, cl, ts, prim = events(rng, 3_000_000, nf, n_nodes)
    labels = rng.integers(0, k, nf)
    nodes = placement(rng, nf, n_nodes, 3)
    load(ctx, f, op, cl, ts, prim)
    ctx.place_evaluate(n_nodes, nodes, k, labels=labels)
    grid = ctx.place_evaluate_info()["workgroups"]
    assert 0 < grid < -(-f.size // WG_CHUNK), "the grid does not saturate: use more events"
    for ne in (grid * WG_CHUNK - 1, grid * WG_CHUNK, grid * WG_CHUNK + 1):
        load(ctx, f[:ne], op[:ne], cl[:ne], ts[:ne], prim)
        compare(ctx, f[:ne], op[:ne], cl[:ne], nodes, n_nodes, k, labels, workgroups=grid)


@pytest.mark.parametrize("nf", [1, 63, 64, 65, 257])
def test_file_counts(ctx, nf):
    rng = np.random.default_rng(nf)
    f, op, cl, ts, prim = events(rng, 5000, nf, 6)
    load(ctx, f, op, cl, ts, prim)
    compare(ctx, f, op, cl, placement(rng, nf, 6, 4), 6, 3, rng.integers(0, 3, nf))


def test_counters_past_16_bits_and_contention(ctx):
    """70 000 READs and 20 000 WRITEs of one client on one file: every lane of
    every wave adds to the same counters."""
    nf = 64
    f = np.full(90_000, 5, dtype=np.int32)
    cl = np.full(90_000, 2, dtype=np.int32)
    op = np.concatenate([np.full(70_000, 2), np.full(20_000, 1)]).astype(np.uint8)
    ts = np.full(f.size, T0, dtype=np.int64)
    prim = np.full(nf, 2, dtype=np.int32)
    load(ctx, f, op, cl, ts, prim)
    nodes = np.full((nf, 3), -1, dtype=np.int32)
    nodes[5] = [0, 2, 1]
    got, _, _ = compare(ctx, f, op, cl, nodes, 3, 1, np.zeros(nf, dtype=np.int64))
    assert got["cluster_sums"].tolist() == [[90_000, 90_000, 70_000, 70_000, 20_000, 60_000]]
    assert got["node_sums"].tolist() == [[0, 0, 0, 20_000, 1], [0, 0, 0, 20_000, 1],
                                         [90_000, 90_000, 70_000, 20_000, 1]]
    pf = ctx.place_evaluate(3, nodes, 1, labels=np.zeros(nf), per_file=True)["per_file"]
    assert pf[5].tolist() == [90_000, 90_000] and pf.sum() == 180_000


def test_identities_with_place_and_the_group_by(ctx):
    """I1 on the device's own placement, I2 against the group-by's
    local_accesses column, I3, on simulated events."""
    nf, n_nodes, k = 20_000, 4, 3
    ne = ctx.features_simulate(nf, 600.0, n_nodes)
    counts, _ = ctx.features_aggregate_resident()
    rng = np.random.default_rng(41)
    labels = rng.integers(0, k, nf)
    placed = ctx.place_replicas(n_nodes, k, [1, 2, 3], 3, labels=labels)
    got = ctx.place_evaluate(n_nodes, placed["nodes"], k, labels=labels, per_file=True)
    np.testing.assert_array_equal(got["per_file"][:, 0], placed["per_file"][:, 0])
    np.testing.assert_array_equal(got["per_file"][:, 1], placed["per_file"][:, 2])
    np.testing.assert_array_equal(got["cluster_sums"][:, 0:2], placed["cluster_sums"][:, [0, 2]])
    np.testing.assert_array_equal(got["node_sums"][:, 4], placed["node_replicas"])
    assert got["node_sums"][:, 1].sum() == got["cluster_sums"][:, 1].sum()
    assert got["cluster_sums"][:, 0].sum() == ne
    f, op, cl, _, prim = ctx.features_events_read()
    only = np.where((prim >= 0) & (prim < n_nodes), prim, -1).reshape(nf, 1)
    got = ctx.place_evaluate(n_nodes, only, k, labels=labels, per_file=True)
    np.testing.assert_array_equal(got["per_file"][:, 1], counts[:, 3])
    np.testing.assert_array_equal(got["per_file"][:, 1], placed["per_file"][:, 1])
    # the simulator's events against the definition
    compare(ctx, f, op, cl, placed["nodes"], n_nodes, k, labels)


def test_events_of_the_device_ingest(ctx):
    import compute_features as cf

    manifest, log = os.path.join(PDIR, "metadata.csv"), os.path.join(PDIR, "access.log")
    paths, _, primary = cf.load_manifest(manifest)
    assert cf.ingest_events(ctx, paths, primary, log) >= 0      # the device tokeniser took it
    n_nodes = len(cf.encode_primary(primary)[1])
    f, op, cl, _, _ = ctx.features_events_read()
    hf, hop, hcl, _, _ = cf.encode(paths, primary, *cf.load_access_log(log))
    rng = np.random.default_rng(51)
    nodes = placement(rng, len(paths), n_nodes, 2)
    labels = rng.integers(0, 2, len(paths))
    compare(ctx, hf, hop, hcl, nodes, n_nodes, 2, labels)
    assert f.size == hf.size


def test_resident_labels_and_untouched_state(ctx):
    import kmeans_plusplus as kp

    rng = np.random.default_rng(13)
    nf, n_nodes, k = 2500, 4, 3
    X = rng.random((nf, 5))
    np.random.seed(0)
    C, labels = kp.kmeans(X, k, random_state=1, context=ctx)
    ctx.agree_keep()
    f, op, cl, ts, prim = events(rng, 60_000, nf, n_nodes)
    load(ctx, f, op, cl, ts, prim)
    rows, _ = ctx.features_aggregate_resident()
    placed = ctx.place_replicas(n_nodes, k, [1, 2, 3], 3, per_file=True, counts=True)

    def state():
        return (ctx.labels(), ctx.medians_by_label(k), ctx.get_rows(np.arange(nf)),
                ctx.agree_table(k, k))

    before = state()
    nodes = placement(rng, nf, n_nodes, 3)
    a, _, _ = compare(ctx, f, op, cl, nodes, n_nodes, k, labels)
    b, _, _ = compare(ctx, f, op, cl, nodes, n_nodes, k, labels, dev_labels="resident")
    np.testing.assert_array_equal(a["cluster_sums"], b["cluster_sums"])
    # k above the resident labels' k is fine, below it is not
    compare(ctx, f, op, cl, nodes, n_nodes, k + 2, labels, dev_labels="resident")
    with pytest.raises(ValueError):
        ctx.place_evaluate(n_nodes, nodes, k - 1)
    for x, y in zip(before, state()):
        np.testing.assert_array_equal(x, y)
    # the events, the group-by's rows and the resident partition
    for x, y in zip((f, op, cl, ts, prim), ctx.features_events_read()):
        np.testing.assert_array_equal(x, y)
    again = ctx.place_replicas(n_nodes, k, [1, 2, 3], 3, per_file=True, counts=True)
    assert ctx.place_info()["reused"] == 1
    for key in ("nodes", "per_file", "counts", "cluster_sums", "node_replicas"):
        np.testing.assert_array_equal(placed[key], again[key])
    rows2, _ = ctx.features_aggregate_resident()
    np.testing.assert_array_equal(rows, rows2)
    t = ctx.place_evaluate_timing()
    assert t.shape == (4,) and (t >= 0).all() and t[2] > 0


def test_errors_leave_the_context_usable(ctx):
    import _cdr

    rng = np.random.default_rng(14)
    nf, n_nodes, k = 500, 3, 2
    f, op, cl, ts, prim = events(rng, 20_000, nf, n_nodes)
    labels = rng.integers(0, k, nf)
    nodes = placement(rng, nf, n_nodes, 2)

    def good(c=ctx):
        compare(c, f, op, cl, nodes, n_nodes, k, labels)

    load(ctx, f, op, cl, ts, prim)
    good()
    for bad_nodes in (0, 65):                                    # CDR_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            ctx.place_evaluate(bad_nodes, nodes, k, labels=labels)
        good()
    for bad_k in (0, 1025):
        with pytest.raises(NotImplementedError):
            ctx.place_evaluate(n_nodes, nodes, bad_k, labels=np.zeros(nf))
        good()
    for width in (0, 9):                                         # CDR_ERR_ARG: R
        with pytest.raises(ValueError):
            ctx.place_evaluate(n_nodes, np.full((nf, width), -1), k, labels=labels)
        good()
    for v in (n_nodes, -2):                                      # a node entry
        bad = nodes.copy()
        bad[17, 1] = v
        with pytest.raises(ValueError):
            ctx.place_evaluate(n_nodes, bad, k, labels=labels)
        good()
    for v in (k, -1):                                            # a label
        bad = labels.copy()
        bad[17] = v
        with pytest.raises(ValueError):
            ctx.place_evaluate(n_nodes, nodes, k, labels=bad)
        good()
    with pytest.raises(ValueError):                              # n_labels != n_files
        ctx.place_evaluate(n_nodes, nodes, k, labels=labels[:-1])
    good()
    # CDR_ERR_STATE: the one-call host aggregate leaves foreign events
    ctx.features_aggregate(f[:100], op[:100], cl[:100], ts[:100], prim)
    with pytest.raises(RuntimeError):
        ctx.place_evaluate(n_nodes, nodes, k, labels=labels)
    load(ctx, f, op, cl, ts, prim)
    good()
    fresh = _cdr.Context(ctx.device)
    try:
        with pytest.raises(RuntimeError):   # no events
            fresh.place_evaluate(3, np.zeros((0, 1)), 1, labels=np.zeros(0))
        assert fresh.place_evaluate_info()["form"] == -1
        fresh.features_load_events(f, op, cl, ts, prim)
        with pytest.raises(RuntimeError):   # no labels on the device
            fresh.place_evaluate(n_nodes, nodes, k)
        good(fresh)
    finally:
        fresh.close()


def test_golden_pipeline_end_to_end(ctx, tmp_path, capsys):
    import compute_features as cf
    import pandas as pd
    import replication_plan
    from replica_placement import (evaluate_from_log, evaluate_host, place_from_log, summary_json,
                                   write_placement_csv)

    t, cats, labels = _golden_inputs(ctx)
    manifest, log = os.path.join(PDIR, "metadata.csv"), os.path.join(PDIR, "access.log")
    facs = t["REPLICATION_FACTORS"]
    res = place_from_log(manifest, log, GOLDEN_CSV, cats, facs, 4, context=ctx)
    yesterday = str(tmp_path / "placement.csv")
    write_placement_csv(yesterday, res["paths"], res["factors"], res["nodes"], res["node_names"])
    # I1 on the same log
    ev = evaluate_from_log(manifest, log, GOLDEN_CSV, yesterday, cats, facs, 4, context=ctx)
    assert ev["paths"] == res["paths"] and ev["node_names"] == res["node_names"]
    np.testing.assert_array_equal(ev["nodes"], res["nodes"][:, :ev["nodes"].shape[1]])
    assert (res["nodes"][:, ev["nodes"].shape[1]:] == -1).all()
    np.testing.assert_array_equal(ev["per_file"], res["per_file"][:, [0, 2]])
    s, p = ev["summary"], res["summary"]
    assert s["events"] == p["events"] and s["local"] == p["local_after"]
    assert s["locality"] == p["locality_after"]
    for cat, row in s["categories"].items():
        assert row["local"] == p["categories"][cat]["local_after"]
    assert [n["replicas"] for n in s["nodes"]] == [n["replicas"] for n in p["nodes"]]
    assert sum(n["local"] for n in s["nodes"]) == s["local"]
    assert s["write_amplification"] is None or s["write_amplification"] >= 1
    # another day's log: every other line
    with open(log) as fh:
        lines = fh.readlines()
    today = str(tmp_path / "today.log")
    with open(today, "w") as fh:
        fh.writelines(lines[::2])
    ev2 = evaluate_from_log(manifest, today, GOLDEN_CSV, yesterday, cats, facs, 4, context=ctx)
    paths, _, primary = cf.load_manifest(manifest)
    f, op, cl, _, _ = cf.encode(paths, primary, *cf.load_access_log(today))
    fpaths = pd.read_csv(GOLDEN_CSV, usecols=["path"], dtype=str)["path"].tolist()
    lab = np.asarray(labels)[[fpaths.index(q) for q in paths]]
    exp = evaluate_host(f, op, cl, ev2["nodes"], len(ev2["node_names"]), labels=lab, k=4)
    np.testing.assert_array_equal(ev2["per_file"], exp["per_file"])
    s2 = ev2["summary"]
    assert s2["events"] == int(exp["cluster_sums"][:, 0].sum()) < s["events"]
    assert s2["write_copies"] == int(exp["cluster_sums"][:, 5].sum())
    assert [[n[key] for key in ("issued", "local", "reads_served", "writes_received", "replicas")]
            for n in s2["nodes"]] == exp["node_sums"].tolist()
    assert s2["unserved_reads"] == exp["unserved_reads"]
    # the CLI prints the same as one more JSON line, and nothing else changes
    capsys.readouterr()

    def run(name, *extra):
        out = str(tmp_path / name)
        np.random.seed(0)
        replication_plan.main(["--input_path", os.path.join(PDIR, "features_out"), "--k", "4",
                               "--tables", os.path.join(PDIR, "main_tables.json"), "--out", out,
                               "--manifest", manifest, *extra], context=ctx)
        with open(out, "rb") as fh:
            return fh.read(), capsys.readouterr().out.replace(out, "OUT")

    plain, plain_text = run("a.csv")
    both, text = run("b.csv", "--access_log", today, "--evaluate_placement", yesterday)
    assert both == plain and text.startswith(plain_text)
    extra = text[len(plain_text):].strip().split("\n")
    assert len(extra) == 1
    # (the CLI's categories come from its own classification of the same clustering)
    line = json.loads(extra[0])
    assert line["node_names"] == ev2["node_names"]
    want = summary_json(s2)
    for key in ("events", "local", "locality", "reads", "reads_local", "writes", "write_copies",
                "write_amplification", "unserved_reads", "read_load_imbalance", "nodes"):
        assert line[key] == json.loads(json.dumps(want[key])), key
    with pytest.raises(SystemExit):
        run("c.csv", "--evaluate_placement", yesterday)

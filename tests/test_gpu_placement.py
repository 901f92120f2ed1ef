"""The replica placement on the device (csrc/place.hip, replica_placement.py)
equals placement_host's integers: node counts, selection, event kinds, counter
widths, every partition shape, the partition's lifetime, both forms, labels,
sizes, errors, untouched state, and end to end on the golden pipeline."""
import csv
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")
GOLDEN_CSV = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
T0 = 1_700_000_000_000_000
NULL = -(2 ** 63)
BUCKET, GLOBAL = 0, 1
SLICE = 12288  # include/cdr.h: the bucket form takes (4 << L) * n_nodes up to this


def events(rng, ne, nf, n_nodes, span_s=600, bad=0.02):
    f = rng.integers(0, nf, ne).astype(np.int32)
    f[rng.random(ne) < bad] = -1
    cl = rng.integers(0, n_nodes, ne).astype(np.int32)
    op = rng.integers(0, 3, ne).astype(np.uint8)
    ts = (T0 + rng.integers(0, max(1, span_s * 1_000_000), ne)).astype(np.int64)
    prim = rng.integers(0, n_nodes, nf).astype(np.int32)
    return f, op, cl, ts, prim


def load(ctx, f, op, cl, ts, prim):
    ctx.features_load_events(f, op, cl, ts, prim)


def compare(ctx, f, cl, prim, n_nodes, k, factors, R, labels, sizes=None, dev_labels="host",
            **want):
    """One place_replicas call over the resident events against the definition."""
    from replica_placement import placement_host

    factors = np.asarray(factors, dtype=np.int32)
    exp = placement_host(f, cl, prim, n_nodes, factors[labels], R, sizes=sizes, labels=labels, k=k)
    got = ctx.place_replicas(n_nodes, k, factors, R, labels=labels if dev_labels == "host" else None,
                             sizes=sizes, per_file=True, counts=True)
    info = ctx.place_info()
    np.testing.assert_array_equal(got["counts"], exp["counts"])
    np.testing.assert_array_equal(got["per_file"], exp["per_file"])
    np.testing.assert_array_equal(got["nodes"], exp["nodes"])
    np.testing.assert_array_equal(got["cluster_sums"], exp["cluster_sums"])
    np.testing.assert_array_equal(got["node_replicas"], exp["node_replicas"])
    assert got["node_bytes"] == exp["node_bytes"]
    for key, v in want.items():
        assert info[key] == v, (key, info)
    return got, info


def simple(ctx, rng, ne, nf, n_nodes, R=3, k=4, span_s=600, **want):
    f, op, cl, ts, prim = events(rng, ne, nf, n_nodes, span_s)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, k, nf)
    factors = rng.integers(0, R + 1, k)
    return compare(ctx, f, cl, prim, n_nodes, k, factors, R, labels, **want)


@pytest.mark.parametrize("n_nodes", [1, 2, 3, 4, 5, 63, 64])
def test_node_counts(ctx, n_nodes):
    rng = np.random.default_rng(n_nodes)
    f, op, cl, ts, prim = events(rng, 60_000, 700, n_nodes)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, 3, 700)
    for R, factors in ((1, [0, 1, 1]), (8, [0, 1, 8]), (3, [3, 2, 1])):
        compare(ctx, f, cl, prim, n_nodes, 3, factors, R, labels, form=BUCKET)


@pytest.mark.parametrize("n_nodes", [0, 65])
def test_node_count_out_of_range(ctx, n_nodes):
    rng = np.random.default_rng(1)
    load(ctx, *events(rng, 100, 10, 3))
    with pytest.raises(NotImplementedError):
        ctx.place_replicas(n_nodes, 1, [1], 1, labels=np.zeros(10))
    compare(ctx, *_resident(ctx), 3, 1, [1], 1, np.zeros(10, dtype=np.int64))


def _resident(ctx):
    f, _, cl, _, prim = ctx.features_events_read()
    return f, cl, prim


def test_selection_rules(ctx):
    """Ties to the lower id, all-zero rows, a null primary, a primary out of
    the node range, a primary with the smallest count still first; a factor
    above n_nodes pads with -1."""
    n_nodes, nf = 5, 9
    ev = ([(0, j) for j in range(5)] * 4                       # all equal: 0, 1, 2, ...
          + [(1, 3)] * 6 + [(1, 1)] * 6 + [(1, 4)] * 2         # tie 1 / 3
          + [(3, 4)] * 5 + [(3, 0)] * 5                        # null primary, tie 0 / 4
          + [(4, 2)] * 9                                       # primary 7: out of range
          + [(5, 0)] * 9 + [(5, 1)] * 8 + [(5, 2)] * 7 + [(5, 3)] * 6 + [(5, 4)] * 1
          + [(6, 1)] * 3 + [(7, 1)] * 3 + [(8, 2)] * 2)
    f = np.array([e[0] for e in ev], dtype=np.int32)
    cl = np.array([e[1] for e in ev], dtype=np.int32)
    prim = np.array([2, 0, 1, -2, 7, 4, 1, -2, 0], dtype=np.int32)
    ts = np.full(f.size, T0, dtype=np.int64)
    load(ctx, f, np.ones(f.size, dtype=np.uint8), cl, ts, prim)
    labels = np.array([0, 0, 0, 0, 0, 0, 1, 2, 3])
    got, _ = compare(ctx, f, cl, prim, n_nodes, 4, [3, 0, 1, 8], 8, labels)
    assert got["nodes"][:6, :3].tolist() == [[2, 0, 1], [0, 1, 3], [1, 0, 2], [0, 4, 1],
                                             [2, 0, 1], [4, 0, 1]]
    assert got["nodes"][8].tolist() == [0, 2, 1, 3, 4, -1, -1, -1]
    assert (got["nodes"][6] == -1).all()


def test_event_kinds(ctx):
    """Paths not in the manifest, clients -1, -3 and past the nodes."""
    rng = np.random.default_rng(7)
    f, op, cl, ts, prim = events(rng, 80_000, 300, 4, bad=0.2)
    cl = rng.choice(np.array([-3, -1, 0, 1, 2, 3, 4, 9, 200], dtype=np.int32), f.size)
    prim = rng.integers(-2, 6, 300).astype(np.int32)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, 4, 300)
    got, _ = compare(ctx, f, cl, prim, 4, 4, [0, 1, 2, 4], 4, labels, form=BUCKET)
    assert got["per_file"][:, 0].sum() > got["counts"].sum() > 0


def test_empty_log_and_all_null_clients(ctx):
    prim = np.array([0, 1, -2, 0, 1, 2, 0, 0, 1, 0], dtype=np.int32)
    e = np.zeros(0, dtype=np.int32)
    load(ctx, e, e.astype(np.uint8), e, e.astype(np.int64), prim)
    labels = np.arange(10) % 2
    got, _ = compare(ctx, e, e, prim, 3, 2, [2, 3], 3, labels)
    assert not got["per_file"].any() and (got["nodes"][:, 0] == [0, 1, 0, 0, 1, 2, 0, 0, 1, 0]).all()
    rng = np.random.default_rng(2)
    f, op, cl, ts, _ = events(rng, 5000, 10, 3)
    cl[:] = -1
    load(ctx, f, op, cl, ts, prim)
    got, _ = compare(ctx, f, cl, prim, 3, 2, [2, 3], 3, labels)
    assert got["per_file"][:, 0].sum() > 0 and not got["per_file"][:, 1:].any()


def test_counters_past_16_bits(ctx):
    rng = np.random.default_rng(3)
    nf = 64
    f = np.concatenate([np.full(70_000, 5), np.arange(nf)]).astype(np.int32)
    cl = np.concatenate([np.full(70_000, 2), np.arange(nf) % 3]).astype(np.int32)
    ts = (T0 + rng.integers(0, 5_000_000, f.size)).astype(np.int64)
    prim = np.full(nf, 2, dtype=np.int32)
    load(ctx, f, np.ones(f.size, dtype=np.uint8), cl, ts, prim)
    got, _ = compare(ctx, f, cl, prim, 3, 1, [1], 1, np.zeros(nf, dtype=np.int64), form=BUCKET)
    assert got["counts"][5, 2] == 70_001 and got["per_file"][5].tolist() == [70_001] * 3


def test_one_bucket_holds_most_of_the_log(ctx):
    rng = np.random.default_rng(4)
    f, op, cl, ts, prim = events(rng, 400_000, 5000, 4)
    f[:360_000] = 1234
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, 3, 5000)
    compare(ctx, f, cl, prim, 4, 3, [1, 2, 3], 3, labels, form=BUCKET)


def test_one_pass_and_L0(ctx):
    _, info = simple(ctx, np.random.default_rng(5), 50_000, 400, 4, form=BUCKET, L=0, buckets=400,
                     payload_bytes=4)
    assert ctx.features_groupby_info()["passes"] == 1


def test_two_passes(ctx):
    _, info = simple(ctx, np.random.default_rng(6), 200_000, 70_001, 4, form=BUCKET,
                     payload_bytes=4)
    gb = ctx.features_groupby_info()
    assert gb["passes"] == 2 and info["L"] == gb["L"]
    assert info["buckets"] == -(-70_001 // (1 << gb["L"])) and 70_001 % (1 << max(gb["L"], 1))


def test_three_passes(ctx, monkeypatch):
    monkeypatch.setenv("CDR_GB_PASS3", "1")
    _, info = simple(ctx, np.random.default_rng(7), 300_000, 300_007, 3, form=BUCKET)
    assert ctx.features_groupby_info()["passes"] == 3


def test_largest_L_and_the_first_past_it(ctx):
    """140 000 files, few events in one second: L = 9.  (4 << 9) * 4 nodes is
    8192 bytes, the bucket form; with 8 nodes it is 16384, past the slice, and
    the global form runs on its own.  The last bucket holds 224 of 512 files."""
    rng = np.random.default_rng(8)
    nf = 140_000
    f, op, cl, ts, prim = events(rng, 6000, nf, 8, span_s=0)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, 4, nf)
    assert (4 << 9) * 4 <= SLICE < (4 << 9) * 8 and nf % 512
    compare(ctx, f, cl, prim, 4, 4, [0, 1, 2, 3], 3, labels, form=BUCKET, L=9,
            buckets=-(-nf // 512))
    _, info = compare(ctx, f, cl, prim, 8, 4, [0, 1, 2, 3], 3, labels, form=GLOBAL)
    assert ctx.features_groupby_info()["L"] == 9


def test_more_than_64_kib_of_lds(ctx):
    """k = 1024 at the L = 9, 4-node shape: 24 672 bytes of sums and four wave
    grids of 10 240 bytes, past the default 64 KiB of dynamic LDS."""
    rng = np.random.default_rng(18)
    nf, k = 140_000, 1024
    f, op, cl, ts, prim = events(rng, 6000, nf, 4, span_s=0)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, k, nf)
    labels[:2] = [0, k - 1]
    assert 24 * (k + 4) + 4 * 4 * 5 * 512 > 64 * 1024
    compare(ctx, f, cl, prim, 4, k, rng.integers(0, 4, k), 3, labels, form=BUCKET, L=9)


def test_eight_byte_payload(ctx):
    # (10 events per file: L = 6, and L + 34 second bits fit the hash key's 40)
    rng = np.random.default_rng(9)
    f, op, cl, ts, prim = events(rng, 400_000, 40_000, 5)
    ts = rng.integers(-(2 ** 31) * 10 ** 6, (2 ** 33) * 10 ** 6, f.size).astype(np.int64)
    ts[:50] = NULL
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, 2, 40_000)
    compare(ctx, f, cl, prim, 5, 2, [2, 5], 5, labels, form=BUCKET, payload_bytes=8)


def test_eight_byte_payload_of_a_dense_partition(ctx):
    """Client ids up to 2^24 (25 client-code bits) make the dense wave
    group-by's payload 41 bits; placement reuses that partition and counts
    every client past the nodes as no node."""
    rng = np.random.default_rng(19)
    nf, wide = 20_000, 1 << 24
    f, op, cl, ts, prim = events(rng, 200_000, nf, 5, span_s=200)
    far = rng.random(f.size) < 0.5
    cl[far] = rng.integers(5, wide, int(far.sum()))
    cl[0] = wide - 1
    load(ctx, f, op, cl, ts, prim)
    ctx.features_aggregate_resident(to_host=False)
    gb = ctx.features_groupby_info()
    assert (gb["hand"], gb["dense"], gb["L"], gb["passes"], gb["payload_bytes"]) == (1, 1, 4, 2, 8), gb
    labels = rng.integers(0, 2, nf)
    compare(ctx, f, cl, prim, 5, 2, [2, 5], 5, labels, form=BUCKET, reused=1, L=4, payload_bytes=8)


def test_last_bucket_writes_nothing_past_n_files(ctx):
    """Guard rows after every host array keep their fill."""
    from _cdr import _check, _ptr
    from replica_placement import placement_host

    rng = np.random.default_rng(10)
    nf, n_nodes, R, k, guard = 1000 + 37, 4, 3, 2, 64
    f, op, cl, ts, prim = events(rng, 3000, nf, n_nodes, span_s=1)
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, k, nf).astype(np.int64)
    factors = np.array([3, 2], dtype=np.int32)
    nodes = np.full((nf + guard, R), -7, dtype=np.int32)
    pf = np.full((nf + guard, 3), -7, dtype=np.int64)
    cnt = np.full((nf + guard, n_nodes), -7, dtype=np.int64)
    cs = np.zeros((k, 3), dtype=np.uint64)
    ns = np.zeros((n_nodes, 3), dtype=np.uint64)
    for env in (None, "1"):
        if env:
            os.environ["CDR_PLACE_GLOBAL"] = env
        try:
            _check(ctx._lib.cdr_place_replicas(ctx._h, n_nodes, _ptr(labels), nf, k, _ptr(factors),
                                               R, None, _ptr(nodes), _ptr(pf), _ptr(cnt), _ptr(cs),
                                               _ptr(ns)))
        finally:
            os.environ.pop("CDR_PLACE_GLOBAL", None)
        info = ctx.place_info()
        assert info["form"] == (GLOBAL if env else BUCKET)
        assert env or (info["L"] >= 1 and nf % (1 << info["L"]))
        exp = placement_host(f, cl, prim, n_nodes, factors[labels], R)
        np.testing.assert_array_equal(nodes[:nf], exp["nodes"])
        np.testing.assert_array_equal(pf[:nf], exp["per_file"])
        np.testing.assert_array_equal(cnt[:nf], exp["counts"])
        assert (nodes[nf:] == -7).all() and (pf[nf:] == -7).all() and (cnt[nf:] == -7).all()


def test_partition_lifetime(ctx):
    rng = np.random.default_rng(11)
    nf, n_nodes, k = 3000, 4, 3
    labels = rng.integers(0, k, nf)
    fac = [1, 2, 3]
    a = events(rng, 100_000, nf, n_nodes)
    b = events(rng, 100_000, nf, n_nodes)       # the same sizes, other events
    load(ctx, *a)
    rows, _ = ctx.features_aggregate_resident()
    compare(ctx, a[0], a[2], a[4], n_nodes, k, fac, 3, labels, form=BUCKET, reused=1)
    compare(ctx, a[0], a[2], a[4], n_nodes, k, fac, 3, labels, form=BUCKET, reused=1)
    rows2, _ = ctx.features_aggregate_resident()
    np.testing.assert_array_equal(rows, rows2)   # the group-by's rows, before and after
    load(ctx, *a)
    compare(ctx, a[0], a[2], a[4], n_nodes, k, fac, 3, labels, form=BUCKET, reused=0)
    compare(ctx, a[0], a[2], a[4], n_nodes, k, fac, 3, labels, form=BUCKET, reused=1)
    load(ctx, *b)                                 # a stale partition would give a's result
    got, _ = compare(ctx, b[0], b[2], b[4], n_nodes, k, fac, 3, labels, form=BUCKET, reused=0)
    rows3, _ = ctx.features_aggregate_resident()
    np.testing.assert_array_equal(got["per_file"][:, 0], rows3[:, 0])
    t = ctx.place_timing()
    assert t.shape == (4,) and (t >= 0).all() and t[2] > 0 and t[0] > 0
    compare(ctx, b[0], b[2], b[4], n_nodes, k, fac, 3, labels, reused=1)
    assert ctx.place_timing()[0] == 0


@pytest.mark.parametrize("env", ["CDR_PLACE_GLOBAL", "CDR_GROUPBY_SORT"])
def test_forms_agree(ctx, monkeypatch, env):
    rng = np.random.default_rng(12)
    nf, n_nodes, k = 20_011, 6, 5
    f, op, cl, ts, prim = events(rng, 300_000, nf, n_nodes)
    cl[rng.random(f.size) < 0.1] = -1
    load(ctx, f, op, cl, ts, prim)
    labels = rng.integers(0, k, nf)
    sizes = rng.integers(0, 2 ** 40, nf)
    fac = [0, 1, 2, 3, 6]
    a, _ = compare(ctx, f, cl, prim, n_nodes, k, fac, 6, labels, sizes=sizes, form=BUCKET)
    monkeypatch.setenv(env, "1")
    b, _ = compare(ctx, f, cl, prim, n_nodes, k, fac, 6, labels, sizes=sizes, form=GLOBAL)
    for key in ("nodes", "per_file", "counts", "cluster_sums", "node_replicas"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["node_bytes"] == b["node_bytes"]


def test_cross_check_with_the_group_by(ctx):
    ne = ctx.features_simulate(20_000, 600.0, 4)
    counts, _ = ctx.features_aggregate_resident()
    got = ctx.place_replicas(4, 1, [2], 2, labels=np.zeros(20_000, dtype=np.int64))
    assert ctx.place_info()["reused"] == 1 and ctx.place_info()["form"] == BUCKET
    np.testing.assert_array_equal(got["per_file"][:, 1], counts[:, 3])
    np.testing.assert_array_equal(got["per_file"][:, 0], counts[:, 0])
    assert got["per_file"][:, 0].sum() == ne
    f, cl, prim = _resident(ctx)
    compare(ctx, f, cl, prim, 4, 1, [2], 2, np.zeros(20_000, dtype=np.int64))


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

    def state():
        return (ctx.labels(), ctx.medians_by_label(k), ctx.get_rows(np.arange(nf)),
                ctx.agree_table(k, k))

    before = state()
    sizes = rng.integers(0, 2 ** 50, nf)
    a, _ = compare(ctx, f, cl, prim, n_nodes, k, [1, 2, 3], 3, labels, sizes=sizes)
    b, _ = compare(ctx, f, cl, prim, n_nodes, k, [1, 2, 3], 3, labels, sizes=sizes,
                   dev_labels="resident")
    np.testing.assert_array_equal(a["nodes"], b["nodes"])
    # k above the resident labels' k is fine, below it is not
    compare(ctx, f, cl, prim, n_nodes, k + 2, [1, 2, 3, 0, 0], 3, labels, dev_labels="resident")
    with pytest.raises(ValueError):
        ctx.place_replicas(n_nodes, k - 1, [1, 2], 3)
    for x, y in zip(before, state()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(before[3], np.diag(np.bincount(labels, minlength=k)))


def test_errors_leave_the_context_usable(ctx):
    import _cdr

    rng = np.random.default_rng(14)
    nf, n_nodes, k = 500, 3, 2
    f, op, cl, ts, prim = events(rng, 20_000, nf, n_nodes)
    labels = rng.integers(0, k, nf)
    sizes = rng.integers(0, 1000, nf)

    def good():
        compare(ctx, f, cl, prim, n_nodes, k, [1, 2], 2, labels, sizes=sizes)

    load(ctx, f, op, cl, ts, prim)
    good()
    bad = labels.copy()
    bad[17] = k
    with pytest.raises(ValueError):
        ctx.place_replicas(n_nodes, k, [1, 2], 2, labels=bad)
    good()
    with pytest.raises(ValueError):
        ctx.place_replicas(n_nodes, k, [1, 3], 2, labels=labels)
    good()
    neg = sizes.copy()
    neg[3] = -1
    with pytest.raises(ValueError):
        ctx.place_replicas(n_nodes, k, [1, 2], 2, labels=labels, sizes=neg)
    good()
    with pytest.raises(ValueError):
        ctx.place_replicas(n_nodes, k, [1, 2], 2, labels=labels[:-1])
    good()
    with pytest.raises(NotImplementedError):
        ctx.place_replicas(n_nodes, 1025, np.ones(1025), 2, labels=labels)
    good()
    # the one-call host aggregate overwrites the buffers without making its
    # events resident: no placement over them until a loader ran
    ctx.features_aggregate(f[:100], op[:100], cl[:100], ts[:100], prim)
    with pytest.raises(RuntimeError):
        ctx.place_replicas(n_nodes, k, [1, 2], 2, labels=labels)
    load(ctx, f, op, cl, ts, prim)
    good()
    fresh = _cdr.Context(ctx.device)
    try:
        with pytest.raises(RuntimeError):   # no events
            fresh.place_replicas(3, 1, [1], 1, labels=np.zeros(0))
        assert fresh.place_info()["form"] == -1
        fresh.features_load_events(f, op, cl, ts, prim)
        with pytest.raises(RuntimeError):   # no labels on the device
            fresh.place_replicas(n_nodes, k, [1, 2], 2)
        compare(fresh, f, cl, prim, n_nodes, k, [1, 2], 2, labels, sizes=sizes, reused=0)
    finally:
        fresh.close()


def test_sizes_past_2_63(ctx):
    rng = np.random.default_rng(15)
    nf, n_nodes = 4000, 3
    f, op, cl, ts, prim = events(rng, 30_000, nf, n_nodes)
    load(ctx, f, op, cl, ts, prim)
    sizes = rng.integers(2 ** 61, 2 ** 63, nf, dtype=np.int64)
    sizes[:5] = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    labels = np.zeros(nf, dtype=np.int64)
    got, _ = compare(ctx, f, cl, prim, n_nodes, 1, [3], 3, labels, sizes=sizes)
    total = sum(int(s) for s in sizes.tolist())
    assert got["node_bytes"] == [total] * 3 and total > 2 ** 63
    assert all(isinstance(b, int) for b in got["node_bytes"])
    got, _ = compare(ctx, f, cl, prim, n_nodes, 1, [3], 3, labels)
    assert got["node_bytes"] == [0, 0, 0]


def _golden_inputs(ctx):
    from features_csv import kmeans_csv

    with open(os.path.join(PDIR, "main_tables.json")) as fh:
        t = json.load(fh)
    np.random.seed(0)
    _, labels = kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)
    cats = {"C0": "Hot", "C1": "Shared", "C2": "Moderate", "C3": "Archival"}
    return t, cats, labels


def test_golden_pipeline_end_to_end(ctx):
    import compute_features as cf
    import pandas as pd
    from replica_placement import place_from_log, placement_host

    t, cats, labels = _golden_inputs(ctx)
    manifest, log = os.path.join(PDIR, "metadata.csv"), os.path.join(PDIR, "access.log")
    res = place_from_log(manifest, log, GOLDEN_CSV, cats, t["REPLICATION_FACTORS"], 4, context=ctx)
    paths, _, primary = cf.load_manifest(manifest)
    f, _, cl, _, prim = cf.encode(paths, primary, *cf.load_access_log(log))
    fpaths = pd.read_csv(GOLDEN_CSV, usecols=["path"], dtype=str)["path"].tolist()
    lab = np.asarray(labels)[[fpaths.index(p) for p in paths]]
    facs = np.array([3, 2, 1, 4])
    sizes = pd.read_csv(manifest)["size_bytes"].to_numpy(dtype=np.int64)
    exp = placement_host(f, cl, prim, 3, facs[lab], 4, sizes=sizes, labels=lab, k=4)
    np.testing.assert_array_equal(res["nodes"], exp["nodes"])
    np.testing.assert_array_equal(res["per_file"], exp["per_file"])
    np.testing.assert_array_equal(res["factors"], facs[lab])
    s = res["summary"]
    assert [n["replicas"] for n in s["nodes"]] == exp["node_replicas"].tolist()
    assert [n["bytes"] for n in s["nodes"]] == exp["node_bytes"]
    assert s["events"] == int(exp["per_file"][:, 0].sum())
    assert s["locality_after"] >= s["locality_before"]
    assert s["locality_after_float"] == float(s["locality_after"])
    assert sum(c["events"] for c in s["categories"].values()) == s["events"]
    assert res["node_names"] == cf.encode_primary(primary)[1] and res["paths"] == paths
    # labels passed from the host, in the features CSV's order, give the same
    again = place_from_log(manifest, log, GOLDEN_CSV, cats, t["REPLICATION_FACTORS"], 4,
                           labels=labels, context=ctx)
    np.testing.assert_array_equal(again["nodes"], res["nodes"])


def test_cli_writes_the_placement(ctx, tmp_path, capsys):
    import replication_plan

    def run(name, *extra):
        out = str(tmp_path / name)
        np.random.seed(0)
        replication_plan.main(["--input_path", os.path.join(PDIR, "features_out"), "--k", "4",
                               "--tables", os.path.join(PDIR, "main_tables.json"), "--out", out,
                               "--manifest", os.path.join(PDIR, "metadata.csv"), *extra],
                              context=ctx)
        with open(out, "rb") as fh:
            return fh.read(), capsys.readouterr().out.replace(out, "OUT")

    plain, plain_text = run("a.csv")
    placement = str(tmp_path / "placement.csv")
    both, text = run("b.csv", "--access_log", os.path.join(PDIR, "access.log"),
                     "--placement", placement)
    assert both == plain and text.startswith(plain_text)
    extra = text[len(plain_text):].strip().split("\n")
    assert len(extra) == 1
    line = json.loads(extra[0])
    with open(placement, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["path", "replication", "nodes"] and len(rows) == 51
    names = line["node_names"]
    plan = {r[0]: r for r in csv.reader(plain.decode().splitlines())}
    # the definition on the host-encoded events, with each file's factor from the plan
    import compute_features as cf
    from replica_placement import placement_host

    paths, _, primary = cf.load_manifest(os.path.join(PDIR, "metadata.csv"))
    f, _, cl, _, prim = cf.encode(paths, primary,
                                  *cf.load_access_log(os.path.join(PDIR, "access.log")))
    assert names == cf.encode_primary(primary)[1]
    factor = np.array([int(plan[p][3]) for p in paths])
    exp = placement_host(f, cl, prim, len(names), factor, int(factor.max()))
    assert [r[0] for r in rows[1:]] == paths
    loads = [0] * len(names)
    for i, (path, rep, nodes) in enumerate(rows[1:]):
        got = [names.index(n) for n in nodes.split(";")] if nodes else []
        assert got == [int(j) for j in exp["nodes"][i] if j >= 0], (i, path)   # same order
        assert len(got) == min(int(rep), len(names)) and plan[path][3] == rep
        for j in got:
            loads[j] += 1
    assert loads == [n["replicas"] for n in line["nodes"]]
    assert 0 < line["locality_before_float"] <= line["locality_after_float"] <= 1
    with pytest.raises(SystemExit):
        run("c.csv", "--placement", placement)

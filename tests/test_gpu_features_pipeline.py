"""GPU parity of the access-log features and the end-to-end main.py flow."""
import glob
import json
import os

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN
from oracle import features_oracle

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")


def test_feature_counts_and_table_match_oracle(ctx, monkeypatch):
    """The golden log in three input orders through the hand-written group-by
    (groupby_resident takes all of them), then the same three under
    CDR_GROUPBY_SORT=1 through the sort fallback: as read (time-ordered: the
    32-bit stable sort by file), shuffled (64-bit (file, second) keys, radix
    sorted) and file-major, second-ordered (64-bit keys, already sorted: no
    sort)."""
    import compute_features as cf

    paths, created, primary = cf.load_manifest(os.path.join(PDIR, "metadata.csv"))
    lt, lp, lo, lc = cf.load_access_log(os.path.join(PDIR, "access.log"))
    fidx, op, cl, ts, prim = cf.encode(paths, primary, lt, lp, lo, lc)
    counts, mx = ctx.features_aggregate(fidx, op, cl, ts, prim)
    exp_counts, exp_mx = features_oracle.counts_from_arrays(fidx, op, cl, ts, prim, len(paths))
    np.testing.assert_array_equal(counts, exp_counts)
    assert mx == exp_mx
    assert ctx.features_groupby_info()["hand"] == 1
    # shuffled input: same counts (the partition is order-independent)
    perm = np.random.default_rng(0).permutation(fidx.size)
    c2, mx2 = ctx.features_aggregate(fidx[perm], op[perm], cl[perm], ts[perm], prim)
    np.testing.assert_array_equal(c2, counts)
    assert ctx.features_groupby_info()["hand"] == 1
    # file-major, second-ordered input: same counts
    order = np.lexsort((ts, fidx))
    c3, _ = ctx.features_aggregate(fidx[order], op[order], cl[order], ts[order], prim)
    np.testing.assert_array_equal(c3, counts)
    assert ctx.features_groupby_info()["hand"] == 1
    # the same three orders through the sort fallback
    with monkeypatch.context() as m:
        m.setenv("CDR_GROUPBY_SORT", "1")
        for o in (np.arange(fidx.size), perm, order):
            cs, mxs = ctx.features_aggregate(fidx[o], op[o], cl[o], ts[o], prim)
            assert ctx.features_groupby_info()["hand"] == 0
            np.testing.assert_array_equal(cs, exp_counts)
            assert mxs == exp_mx
    table = ctx.features_finalize(counts, created, mx / 1e6)
    z = np.load(os.path.join(PDIR, "features_oracle.npz"))
    np.testing.assert_array_equal(table, z["table"])
    np.testing.assert_array_equal(table, features_oracle.finalize(counts, created, mx / 1e6))


def test_random_event_logs_exact(ctx):
    rng = np.random.default_rng(5)
    nf, ne = 5000, 200000
    prim = rng.integers(-2, 4, nf).astype(np.int32)
    fidx = rng.integers(-1, nf, ne).astype(np.int32)
    op = rng.integers(0, 3, ne).astype(np.uint8)
    cl = rng.integers(-1, 4, ne).astype(np.int32)
    ts = (1_700_000_000_000_000 + rng.integers(-5_000_000, 600_000_000, ne)).astype(np.int64)
    got, mx = ctx.features_aggregate(fidx, op, cl, ts, prim)
    exp, emx = features_oracle.counts_from_arrays(fidx, op, cl, ts, prim, nf)
    np.testing.assert_array_equal(got, exp)
    assert mx == emx
    cr = np.where(rng.random(nf) < 0.05, np.nan, 1.69e9 + rng.integers(0, 10**6, nf)).astype(float)
    np.testing.assert_array_equal(ctx.features_finalize(got, cr, mx / 1e6),
                                  features_oracle.finalize(got, cr, mx / 1e6))


def test_compute_features_cli_writes_spark_layout(ctx, tmp_path):
    import compute_features as cf

    out = tmp_path / "features_out"
    cf.main(["--manifest", "file://" + os.path.join(PDIR, "metadata.csv"),
             "--access_log", os.path.join(PDIR, "access.log"), "--out", str(out)])
    parts = glob.glob(str(out / "part-00000*.csv"))
    assert len(parts) == 1
    got = pd.read_csv(parts[0], float_precision="round_trip")
    golden = pd.read_csv(glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0],
                         float_precision="round_trip")
    pd.testing.assert_frame_equal(got, golden)
    with open(parts[0]) as fh, open(glob.glob(os.path.join(PDIR, "features_out",
                                                            "part-00000*.csv"))[0]) as gh:
        assert fh.read() == gh.read()


def test_main_py_flow_matches_reference(ctx):
    """src/main.py:75-142 driven through the drop-in modules: same kmeans call
    (:91), same list building (:96-102), same classifier (:106-107)."""
    import kmeans_plusplus as kp
    from scoring import ClusterClassifier

    with open(os.path.join(PDIR, "main_tables.json")) as fh:
        t = json.load(fh)
    feats = t["CLUSTERING_FEATURES"]
    path = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
    df = pd.read_csv(path)  # main.py:75 uses the default parser
    X = df[feats].values
    C, labels = kp.kmeans(X, 4, number_of_files=len(df), random_state=42, context=ctx)
    ref = np.load(os.path.join(PDIR, "main_kmeans.npz"))
    np.testing.assert_array_equal(labels, ref["labels"])
    np.testing.assert_array_equal(C, ref["centroids"])
    df["cluster"] = labels
    data = {f"C{i}": {f: df[df["cluster"] == i][f].tolist() for f in feats} for i in range(4)}
    clf = ClusterClassifier(t["GLOBAL_MEDIANS"], t["WEIGHTS"], t["DIRECTIONS"],
                            t["REPLICATION_FACTORS"], context=ctx)
    cats = clf.classify(data)
    final = pd.read_csv(os.path.join(PDIR, "final_categories.csv"), float_precision="round_trip")
    assert [cats[f"C{i}"] for i in range(4)] == list(final["category"])
    np.testing.assert_array_equal(C, final[feats].to_numpy())


def test_generated_log_exact(ctx):
    """Device-generated, time-ordered log (the config-4 generator): the
    resident group-by (the hand-written partition and bucket kernels) equals
    the independent oracle counters and the host-upload path, bit for bit."""
    ne, nf = 3_000_000, 300_000
    ctx.features_generate(ne, nf, seed=1234)
    got, mx = ctx.features_aggregate_resident()
    assert ctx.features_groupby_info()["hand"] == 1
    f, op, cl, ts, pr = ctx.features_events_read()
    assert np.all(np.diff(ts) >= 0)  # time-ordered, as the generator promises
    want, wmx = features_oracle.counts_from_arrays(f, op, cl, ts, pr, nf)
    np.testing.assert_array_equal(got, want)
    assert mx == wmx
    up, umx = ctx.features_aggregate(f, op, cl, ts, pr)
    np.testing.assert_array_equal(up, want)
    assert ctx.features_groupby_info()["hand"] == 1


def test_generated_log_config4_shard(ctx):
    """One GPU's share of config 4 (1B events over 8 GPUs): 125M events over
    12.5M files.  Counters checked exactly with bincount; max_concurrency
    exactly through unique (file, second) keys."""
    ne, nf = 125_000_000, 12_500_000
    ctx.features_generate(ne, nf, seed=99)
    got, mx = ctx.features_aggregate_resident()
    f, op, cl, ts, pr = ctx.features_events_read()
    f64 = f.astype(np.int64)
    np.testing.assert_array_equal(got[:, 0], np.bincount(f64, minlength=nf))
    np.testing.assert_array_equal(got[:, 1], np.bincount(f64, weights=(op == 1), minlength=nf))
    np.testing.assert_array_equal(got[:, 2], np.bincount(f64, weights=(op == 2), minlength=nf))
    np.testing.assert_array_equal(got[:, 3], np.bincount(f64, weights=(cl == pr[f]), minlength=nf))
    np.testing.assert_array_equal(got[:, 4], got[:, 0])
    assert got[:, 0].sum() == ne and mx == int(ts.max())
    sec = ts // 1_000_000  # ts > 0: floor division == floor(ts / 1e6) here
    key = f64 * 1024 + (sec - sec.min())
    del sec
    uk, cnt = np.unique(key, return_counts=True)
    conc = np.zeros(nf, dtype=np.int64)
    np.maximum.at(conc, uk // 1024, cnt)
    np.testing.assert_array_equal(got[:, 5], conc)


@pytest.mark.parametrize("ne,nf", [(0, 5), (1, 1), (2, 3), (70_000, 1)])
def test_generated_log_edge_sizes(ctx, monkeypatch, ne, nf):
    """Empty and tiny logs, a single manifest file (fbits edge) on the
    resident path: same counters as the oracle, from the hand-written
    group-by and then, under CDR_GROUPBY_SORT=1, from the sort fallback."""
    ctx.features_generate(ne, nf, seed=ne + nf)
    got, mx = ctx.features_aggregate_resident()
    assert ctx.features_groupby_info()["hand"] == 1
    f, op, cl, ts, pr = ctx.features_events_read()
    want, wmx = features_oracle.counts_from_arrays(f, op, cl, ts, pr, nf)
    np.testing.assert_array_equal(got, want)
    if ne:
        assert mx == wmx
    monkeypatch.setenv("CDR_GROUPBY_SORT", "1")
    got, mx = ctx.features_aggregate_resident()
    assert ctx.features_groupby_info()["hand"] == 0
    np.testing.assert_array_equal(got, want)
    if ne:
        assert mx == wmx

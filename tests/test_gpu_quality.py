"""Silhouette and Davies-Bouldin on the device (csrc/quality.hip,
cluster_quality.py) against the NumPy model tests/quality_model.py.

Tile sizes of the pair kernel: a workgroup takes 256 rows for d <= 32 and 128
rows for d > 32 (128 threads with two rows or one row each), and the columns
come in LDS tiles of 64.  The sizes below therefore include T - 1, T, T + 1 for
T = 64, 128 and 256, next to the smallest and some ordinary ones.

Tolerance (derived, not measured): each side's a_i and b_i carry a relative
error of at most eps = (m + d/2 + 2) u, u = 2^-53: d + 2 roundings under the
square root (which halves them), the root, fewer than m additions of
non-negative terms in any order, one division.  Each side's s_i is then off
by at most 2 eps + 4 u, so the comparison is atol = 4 (m + d/2 + 6) u, rtol 0,
for s, the score and the per-cluster means.  Davies-Bouldin sums: relative
2 (n + d/2 + 2) u per cluster.
"""
import os
import re

import numpy as np
import pytest

import quality_model as qm
from conftest import PKG
from oracle import synth

pytestmark = pytest.mark.gpu

MODE_F32X, MODE_F64 = 1, 2
SIZES = (3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2048)


def _points(mode, n, d, seed):
    if mode == MODE_F32X:
        return synth.generate(n, 0, n, d, 4, seed)
    return np.random.default_rng(seed).random((n, d))


def _labels(rng, m, k):
    """Random labels in [0, k); rows 0, 1 share cluster 0 and row 2 is in
    cluster 1, so that at least 2 and at most m - 1 clusters are non-empty."""
    lab = rng.integers(0, k, size=m).astype(np.int64)
    lab[:3] = (0, 0, 1)
    return lab


def _compare(ctx, X, labels, k, mode, idx=None):
    import cluster_quality as cq

    ctx.load_points(X)
    assert ctx.info()["mode"] == mode
    Xs, ls = (X, labels) if idx is None else (X[idx], labels[idx])
    m, d = Xs.shape
    score, per, s, ind = cq.silhouette(labels=labels, k=k, indices=idx, context=ctx)
    s_ref, csum_ref, cnt_ref = qm.silhouette_samples(Xs, ls, k)
    atol = qm.sil_atol(m, d)
    err = np.abs(s - s_ref).max()
    print(f"m={m} d={d} k={k} mode={mode}: max |s - model| = {err:.3e} (atol {atol:.3e})")
    np.testing.assert_allclose(s, s_ref, rtol=0, atol=atol)
    assert abs(score - np.mean(s_ref)) <= atol
    with np.errstate(invalid="ignore", divide="ignore"):
        per_ref = csum_ref / cnt_ref
    assert np.array_equal(np.isnan(per), cnt_ref == 0)
    np.testing.assert_allclose(per[cnt_ref > 0], per_ref[cnt_ref > 0], rtol=0, atol=atol)
    assert np.array_equal(ind, np.arange(m) if idx is None else idx)
    return s


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
@pytest.mark.parametrize("d", (5, 64))
@pytest.mark.parametrize("m", SIZES)
def test_silhouette_sizes(ctx, m, d, mode):
    rng = np.random.default_rng(1000 * m + d)
    _compare(ctx, _points(mode, m, d, 7 * m + d), _labels(rng, m, 4), 4, mode)


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
@pytest.mark.parametrize("d", (1, 5, 16, 17, 24, 64))
def test_silhouette_dims(ctx, d, mode):
    rng = np.random.default_rng(d)
    _compare(ctx, _points(mode, 257, d, 31 + d), _labels(rng, 257, 4), 4, mode)


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
@pytest.mark.parametrize("k", (2, 4, 64, 300))
def test_silhouette_ks(ctx, k, mode):
    rng = np.random.default_rng(k)
    _compare(ctx, _points(mode, 1000, 16, 77 + k), _labels(rng, 1000, k), k, mode)


@pytest.mark.parametrize("d", (5, 64))
def test_row_range_split_over_launches(ctx, d, monkeypatch):
    """The pair budget splits the row range over several launches; a small
    budget (CDR_QUALITY_BUDGET can only lower it) reaches that at m = 1000:
    row tiles of 256 (d = 5) and 128 (d = 64), the last launch partly filled."""
    monkeypatch.setenv("CDR_QUALITY_BUDGET", "300000")
    rng = np.random.default_rng(d)
    _compare(ctx, _points(MODE_F64, 1000, d, 5 + d), _labels(rng, 1000, 7), 7, MODE_F64)
    assert ctx.quality_timing()["pair_launches"] == 4
    monkeypatch.delenv("CDR_QUALITY_BUDGET")
    _compare(ctx, _points(MODE_F64, 1000, d, 5 + d), _labels(rng, 1000, 7), 7, MODE_F64)
    assert ctx.quality_timing()["pair_launches"] == 1


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
def test_cluster_sizes_one_tile_and_empty_ids(ctx, mode):
    """Clusters of 1, 64 (one column tile) and 65 rows; label ids 2 (middle)
    and 5 = k - 1 empty; rows not grouped by label."""
    rng = np.random.default_rng(5)
    labels = np.repeat(np.array([0, 1, 3, 4]), [1, 64, 65, 127])
    rng.shuffle(labels)
    s = _compare(ctx, _points(mode, 257, 5, 99), labels, 6, mode)
    assert s[labels == 0][0] == 0.0  # the singleton, exactly


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
def test_identical_points_score_exactly_one(ctx, mode):
    """Every row of cluster 0 is the same point (each row of the data twice
    over, as data_families' const_dup): a_i = 0 exactly, so s_i == 1.0.  A
    Gram-form distance gives ~1e-8 instead of 0 and fails this."""
    import cluster_quality as cq

    X = np.concatenate([np.repeat(_points(mode, 1, 7, 3), 66, axis=0), _points(mode, 70, 7, 4),
                        _points(mode, 1, 7, 8)])
    labels = np.repeat(np.array([0, 1, 2]), [66, 70, 1])
    ctx.load_points(X)
    assert ctx.info()["mode"] == mode
    _, _, s, _ = cq.silhouette(labels=labels, k=3, context=ctx)
    assert np.all(s[:66] == 1.0)
    assert s[-1] == 0.0  # singleton
    _, _, s2, _ = cq.silhouette(labels=labels, k=3, context=ctx)
    assert np.array_equal(s, s2)


def test_two_calls_are_bit_identical(ctx):
    import cluster_quality as cq

    X = _points(MODE_F64, 1000, 16, 12)
    labels = _labels(np.random.default_rng(1), 1000, 64)
    ctx.load_points(X)
    a = cq.silhouette(labels=labels, k=64, context=ctx)
    b = cq.silhouette(labels=labels, k=64, context=ctx)
    assert a[0] == b[0] and np.array_equal(a[2], b[2])
    assert np.array_equal(a[1], b[1], equal_nan=True)
    C = qm.cluster_means(X, labels, 64)
    s1, c1 = ctx.quality_scatter(C, labels)
    s2, c2 = ctx.quality_scatter(C, labels)
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2)


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
def test_callers_row_order(ctx, mode):
    """Shuffled, repeat-free indices with caller labels: s comes back in the
    order given, not in sorted or label order."""
    rng = np.random.default_rng(17)
    X = _points(mode, 700, 5, 21)
    labels = _labels(rng, 700, 4)
    idx = rng.permutation(700)[:300].astype(np.int64)
    s = _compare(ctx, X, labels, 4, mode, idx=idx)
    order = np.argsort(idx)
    s_sorted = _compare(ctx, X, labels, 4, mode, idx=idx[order])
    # (another row order is another summation order: equal within the bound only)
    np.testing.assert_allclose(s[order], s_sorted, rtol=0, atol=qm.sil_atol(300, 5))
    assert np.abs(s - s_sorted).max() > 1e-3  # the given order is not the sorted one


@pytest.fixture(scope="module")
def fitted():
    """kmeans(X, 4, max_iter=20, random_state=42) on 5000 x 5 in a context of
    its own: (ctx, X, centroids, labels)."""
    import _cdr
    import kmeans_plusplus as kp

    c = _cdr.Context(int(os.environ.get("CDR_DEVICE", "0")))
    X = synth.generate(5000, 0, 5000, 5, 4, 0xC0FFEE)
    np.random.seed(0)
    C, labels = kp.kmeans(X, 4, max_iter=20, random_state=42, context=c)
    yield c, X, C, labels
    c.close()


def test_resident_labels_silhouette(fitted):
    import cluster_quality as cq

    c, X, C, labels = fitted
    score, per, s, ind = cq.silhouette(context=c)
    s_ref, csum, cnt = qm.silhouette_samples(X, labels, 4)
    atol = qm.sil_atol(5000, 5)
    np.testing.assert_allclose(s, s_ref, rtol=0, atol=atol)
    assert abs(score - s_ref.mean()) <= atol
    np.testing.assert_allclose(per, csum / cnt, rtol=0, atol=atol)
    assert np.array_equal(ind, np.arange(5000))


def test_resident_labels_davies_bouldin(fitted):
    import cluster_quality as cq

    c, X, C, labels = fitted
    sums, counts = c.quality_scatter(C)
    sums_ref, counts_ref = qm.scatter(X, labels, C)
    assert np.array_equal(counts, counts_ref)
    np.testing.assert_allclose(sums, sums_ref, rtol=qm.scatter_rtol(5000, 5), atol=0)
    db = cq.davies_bouldin(C, context=c)
    # DB is a mean of ratios of those sums (exactly the same host arithmetic on
    # both sides otherwise): relative error within twice the sums' (numerator
    # and the division by the counts)
    assert abs(db - qm.davies_bouldin(X, labels, C)) <= 2 * qm.scatter_rtol(5000, 5) * db


def test_sampling(fitted):
    import cluster_quality as cq

    c, X, C, labels = fitted
    score, per, s, ind = cq.silhouette(sample_size=500, random_state=7, context=c)
    want = np.sort(np.random.default_rng(7).choice(5000, size=500, replace=False))
    assert np.array_equal(ind, want)
    s_ref, _, _ = qm.silhouette_samples(X[want], labels[want], 4)
    np.testing.assert_allclose(s, s_ref, rtol=0, atol=qm.sil_atol(500, 5))


@pytest.mark.parametrize("mode", (MODE_F32X, MODE_F64))
@pytest.mark.parametrize("n,d,k", [(3, 1, 3), (1023, 5, 4), (1025, 17, 64), (5000, 64, 300),
                                   (20000, 16, 300)])
def test_scatter_shapes(ctx, n, d, k, mode):
    """Chunks of 1024 rows: below, across and many; centroids in LDS
    (k d <= 6144) and in global memory; an empty id in the middle and at k - 1."""
    rng = np.random.default_rng(n + d + k)
    X = _points(mode, n, d, n + 1)
    labels = _labels(rng, n, k - 1)
    if k > 3:
        labels[labels == k // 2] = 0
    C = rng.random((k, d))
    ctx.load_points(X)
    assert ctx.info()["mode"] == mode
    sums, counts = ctx.quality_scatter(C, labels)
    sums_ref, counts_ref = qm.scatter(X, labels, C)
    assert np.array_equal(counts, counts_ref)
    assert counts[k - 1] == 0 and sums[k - 1] == 0.0
    np.testing.assert_allclose(sums, sums_ref, rtol=qm.scatter_rtol(n, d), atol=0)


def test_sweep_rows_equal_separate_calls():
    import _cdr
    import cluster_quality as cq
    import kmeans_plusplus as kp

    c = _cdr.Context(int(os.environ.get("CDR_DEVICE", "0")))
    try:
        X = synth.generate(5000, 0, 5000, 5, 4, 0xC0FFEE)
        np.random.seed(0)
        rows = cq.sweep(X, [2, 3, 4], random_state=42, max_iter=20, context=c)
        assert [r["k"] for r in rows] == [2, 3, 4]
        np.random.seed(0)
        for r in rows:
            C, labels = kp.kmeans(X, r["k"], max_iter=20, random_state=42, context=c)
            assert r["silhouette"] == cq.silhouette(k=r["k"], random_state=42, context=c)[0]
            assert r["davies_bouldin"] == cq.davies_bouldin(C, context=c)
            assert r["nonempty"] == np.unique(labels).size
            assert r["inertia"] == c.last_inertia and r["inertia"] is not None
        assert rows[0]["inertia"] > rows[1]["inertia"] > rows[2]["inertia"]
    finally:
        c.close()


def test_errors(ctx):
    import _cdr
    import cluster_quality as cq

    X = _points(MODE_F64, 100, 5, 1)
    ctx.load_points(X)
    with pytest.raises(ValueError):  # one non-empty cluster
        cq.silhouette(labels=np.zeros(100, dtype=np.int64), k=4, context=ctx)
    with pytest.raises(ValueError):  # every row its own cluster: more than m - 1
        cq.silhouette(labels=np.arange(100), k=100, context=ctx)
    with pytest.raises(ValueError):  # m = 2 leaves no admissible cluster count
        cq.silhouette(labels=np.arange(100) % 2, k=2, indices=[0, 1], context=ctx)
    with pytest.raises(ValueError):  # label >= k
        cq.silhouette(labels=np.arange(100) % 5, k=4, context=ctx)
    with pytest.raises(ValueError):
        ctx.quality_scatter(np.zeros((4, 5)), np.arange(100) % 5)
    with pytest.raises(ValueError):  # row out of range
        ctx.silhouette(2, idx=[0, 1, 100], labels=[0, 0, 1])
    with pytest.raises(ValueError):  # one non-empty cluster
        cq.davies_bouldin(np.zeros((3, 5)), labels=np.zeros(100, dtype=np.int64), context=ctx)
    with pytest.raises(NotImplementedError):
        cq.silhouette(labels=np.arange(100) % 2, context=ctx, comm=object())
    ctx.load_points(_points(MODE_F64, 10, 65, 2))
    with pytest.raises(NotImplementedError):  # d = 65
        cq.silhouette(labels=np.arange(10) % 2, k=2, context=ctx)
    with pytest.raises(NotImplementedError):
        ctx.quality_scatter(np.zeros((2, 65)), np.arange(10) % 2)
    fresh = _cdr.Context(ctx.device)
    try:
        with pytest.raises(RuntimeError):  # no points at all
            fresh.silhouette(2)
        fresh.load_points(X)
        with pytest.raises(RuntimeError):  # points, but no labels on the device
            cq.silhouette(k=2, context=fresh)
        with pytest.raises(RuntimeError):
            cq.davies_bouldin(np.zeros((2, 5)), context=fresh)
    finally:
        fresh.close()


def test_cluster_quality_does_not_import_oracle():
    with open(os.path.join(PKG, "cluster_quality.py")) as fh:
        src = fh.read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M)

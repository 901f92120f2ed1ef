"""The medians of all resident points (csrc/medians.hip gm_hist32 / gm_hist64,
Context.medians_global, the pass API, cdr_dist.sharded_global_medians and
scoring.global_medians / ClusterClassifier.from_points) against np.median of
the same table.

Every comparison is exact: np.testing.assert_array_equal plus the sign bit
(a median is never -0.0).  The tables come from tests/global_median_cases.py,
whose CPU test checks that each is what it claims."""
import glob
import os
import threading

import numpy as np
import pytest

import data_families as df
import global_median_cases as gc
import median_cases as mc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GM_ROWS = 512  # kGmRows (csrc/medians.hip): rows one wave takes per turn
MODE = {"f32x": mc.MODE_F32X, "f64": mc.MODE_F64}


def _same(got, exp):
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))


def _check(ctx, name):
    X, exp = gc.case(name)
    ctx.load_points(X)
    if name != "minmax":
        assert ctx.info()["mode"] == MODE[name.rsplit("-", 1)[1]], ctx.info()
    got = ctx.medians_global()
    assert got.shape == (X.shape[1],) and got.dtype == np.float64
    _same(got, exp)
    return X, exp, got


# ---- 1. rows ---------------------------------------------------------------
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("n", gc.ROW_N)
def test_row_edges(ctx, n, mode):
    """n at the wave width, at kGmRows - 1, + 0, + 1 (one wave turn), at a whole
    workgroup turn and at the 8192-row padding: every value lies in [1, 2), so
    one counted padding row (a zero) lowers a median."""
    assert gc.GM_ROWS == GM_ROWS
    _check(ctx, "rows-%d-%s" % (n, mode))


@pytest.mark.parametrize("mode", gc.MODES)
def test_grid_stride(ctx, mode, monkeypatch):
    """CDR_GMED_GRID=3 (it can only lower the workgroup cap): 12 waves take the
    137 row groups of 70 001 rows (x 2 quads, or x 5 features) in many turns,
    the last group partial; the result is the default grid's."""
    assert -(-gc.GRID_N // GM_ROWS) > 10 * 3 * gc.GM_WAVES and gc.GRID_N % GM_ROWS
    monkeypatch.delenv("CDR_GMED_GRID", raising=False)
    X, exp, got = _check(ctx, "grid-" + mode)
    monkeypatch.setenv("CDR_GMED_GRID", "3")
    _same(ctx.medians_global(), got)
    monkeypatch.setenv("CDR_GMED_GRID", "1000000")  # above the cap: no effect
    _same(ctx.medians_global(), got)


# ---- 2. features -----------------------------------------------------------
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("d", gc.FEAT_D)
def test_feature_edges(ctx, d, mode):
    """The quad padding of x32 (d = 1, 2, 3, 5), both sides of every boundary
    of the 16-feature chunks (16 | 17, 64 | 65), a column alone in its chunk
    (17, 65) and eight chunks (128)."""
    _check(ctx, "feat-%d-%s" % (d, mode))


# ---- 3. where the ranks part, degenerate digits ----------------------------
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("n", gc.PART_N)
def test_where_the_ranks_part(ctx, n, mode):
    """Even and odd n with planted columns: middle values equal, neighbours, of
    opposite sign, -0.0 / +0.0 (F64), and first differing in each key byte."""
    X, exp, got = _check(ctx, "part-%d-%s" % (n, mode))
    notes = [nt[0] for nt in gc.part_notes(mode)]
    assert sum(nt.startswith("byte") for nt in notes) == (4 if mode == "f32x" else 8)
    if n % 2 == 0:
        assert got[notes.index("opposite sign")] == 0.0 and got[notes.index("equal")] == 0.125
        if mode == "f64":
            z = got[notes.index("signed zeros")]
            assert z == 0 and not np.signbit(z)


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("n", gc.DEGEN_N)
def test_degenerate_digits(ctx, n, mode):
    """A constant column, two values 1:1 and 1:(n-1), half one value and the
    rest random, and a constant column whose quad neighbours are random (the
    lanes of a wave disagree on whether their digit is uniform)."""
    X, exp, got = _check(ctx, "degen-%d-%s" % (n, mode))
    assert got[0] == 0.375 and got[2] == 0.25 and got[3] == 0.5 and got[5] == 0.625
    assert got[1] == (0.5 if n % 2 == 0 else 0.75)


# ---- 4. data outside the unit cube, the golden CSV, float32 input ----------
@pytest.mark.parametrize("d", [5, 16])
@pytest.mark.parametrize("name", df.FAMILIES)
def test_data_families(ctx, name, d):
    X = df.family(name, 12_000, d, 700 + d)
    ctx.load_points(X)
    if df.EXPECT[name] is not None:
        assert ctx.info()["mode"] == df.EXPECT[name][0], ctx.info()
    _same(ctx.medians_global(), np.median(X, axis=0))


def test_family_scales_seen():
    """The F32X families load with S = 0, 12, 14, 24 and 126."""
    assert {v[1] for v in df.EXPECT.values() if v and v[0] == mc.MODE_F32X} == {0, 12, 14, 24, 126}


def test_golden_features_csv(ctx):
    import pandas as pd

    import csv_read_cases as rc
    from features_csv import read_features

    path = glob.glob(os.path.join(GOLDEN, "pipeline", "features_out", "part-00000*.csv"))[0]
    info = {}
    read_features(path, ctx=ctx, info=info)
    assert info["resident"], info
    want = pd.read_csv(path)[rc.FEATURES]
    _same(ctx.medians_global(), np.array([np.median(want[c]) for c in rc.FEATURES]))


@pytest.mark.parametrize("grid", [True, False])
def test_float32_input(ctx, grid):
    """float32 X through kmeans_plusplus' own load path: the medians are those
    of the float64 conversions."""
    import kmeans_plusplus as kp

    rng = np.random.default_rng(61)
    X = rng.normal(0, 2, (9001, 6)).astype(np.float32)
    if grid:
        X = (np.round(X * 1024) / 1024).astype(np.float32)
    kp.kmeans_plusplus_init(X, 3, random_state=5, context=ctx)
    if grid:
        assert ctx.info()["mode"] == mc.MODE_F32X
    _same(ctx.medians_global(), np.median(X.astype(np.float64), axis=0))


# ---- 5. state ----------------------------------------------------------------
def test_no_points_and_no_rows():
    import _cdr

    c = _cdr.Context(0)
    try:
        with pytest.raises(RuntimeError, match="no points"):
            c.medians_global()
        with pytest.raises(RuntimeError, match="no points"):
            c.medians_global_begin(10)
        c.load_points(np.empty((0, 3)))
        got = c.medians_global()
        assert got.shape == (3,) and np.isnan(got).all()
    finally:
        c.close()


def test_before_any_step_and_twice(ctx):
    X, exp = gc.case("minmax")
    ctx.load_points(X)
    a = ctx.medians_global()
    b = ctx.medians_global()
    _same(a, exp)
    _same(b, a)
    tm = ctx.medians_global_timing()
    assert tm["passes"] == 8 and tm["hist_ms"] >= tm["hist_max_ms"] > 0


def test_after_kmeans_f32x_device_loop(ctx):
    import kmeans_plusplus as kp

    rng = np.random.default_rng(47)
    X = np.floor(rng.random((24_539, 7)) * 2.0 ** 24) * 2.0 ** -24
    np.random.seed(0)
    _, lab = kp.kmeans(X, 20, random_state=42, max_iter=8, context=ctx)
    assert ctx.info()["mode"] == mc.MODE_F32X
    _same(ctx.medians_global(), np.median(X, axis=0))
    # labels, running state and the cluster medians are untouched
    np.testing.assert_array_equal(ctx.labels(), lab)
    np.testing.assert_array_equal(ctx.medians_by_label(20), mc.ref_medians(X, lab, 20))


def test_after_kmeans_f64_run(ctx):
    import kmeans_plusplus as kp

    X, exp = gc.case("minmax")
    np.random.seed(0)
    _, lab = kp.kmeans(X, 4, random_state=42, context=ctx)
    assert ctx.info()["mode"] == mc.MODE_F64
    _same(ctx.medians_global(), exp)
    np.testing.assert_array_equal(ctx.labels(), lab)
    np.testing.assert_array_equal(ctx.medians_by_label(4), mc.ref_medians(X, lab, 4))


@pytest.mark.parametrize("name", ["stale_a-f32x", "stale_a-f64"])
def test_between_group_and_begin(ctx, name):
    """cdr_medians_group -> global medians (one call, then the pass calls
    interleaved with the cluster passes) -> cdr_medians_begin / passes /
    finish: both results are right, neither disturbs the other."""
    X, C, lab, sizes = mc.case(name)
    ctx.load_points(X)
    (ctx.lloyd_step if name.endswith("f32x") else ctx.lloyd_step_f64)(C)
    counts = ctx.medians_group(3)
    exp = np.median(X, axis=0)
    _same(ctx.medians_global(), exp)
    gp, gwords = ctx.medians_global_begin(X.shape[0])
    passes, words = ctx.medians_begin(counts)
    assert gp == passes and gwords == X.shape[1] * 512
    h, gh = np.zeros(words, dtype=np.uint32), np.zeros(gwords, dtype=np.uint32)
    for p in range(passes):
        ctx.medians_pass_hist(p, h)
        ctx.medians_global_pass_hist(p, gh)
        assert int(gh.reshape(-1, 2, 256)[:, 0].sum()) <= X.size
        ctx.medians_pass_select(p, h)
        ctx.medians_global_pass_select(p, gh)
    np.testing.assert_array_equal(ctx.medians_finish(), mc.ref_medians(X, lab, 3))
    _same(ctx.medians_global_finish(), exp)


def test_begun_state_ends_with_new_points_not_with_a_step(ctx):
    X, C, lab, _ = mc.case("stale_a-f32x")
    X2, _, _, _ = mc.case("stale_b-f32x")
    ctx.load_points(X)
    passes, words = ctx.medians_global_begin(X.shape[0])
    ctx.lloyd_step(C)  # nothing here depends on the labels
    h = np.zeros(words, dtype=np.uint32)
    for p in range(passes):
        ctx.medians_global_pass_hist(p, h)
        ctx.medians_global_pass_select(p, h)
    _same(ctx.medians_global_finish(), np.median(X, axis=0))
    with pytest.raises(ValueError):
        ctx.medians_global_pass_hist(passes, h)
    ctx.load_points(X2)
    for call in (lambda: ctx.medians_global_pass_hist(0, h),
                 lambda: ctx.medians_global_pass_select(0, h), ctx.medians_global_finish):
        with pytest.raises(RuntimeError, match="cdr_medians_global_begin"):
            call()
    _same(ctx.medians_global(), np.median(X2, axis=0))


# ---- 6. the pass API over shards, several contexts on one GPU ---------------
def _unify(ctxs, n_total):
    """cdr_dist.unify_points with the MIN / MAX all-reduce done here."""
    sts = [c.points_stats() for c in ctxs]
    dd = (sts[0].size - 3) // 2
    g = np.concatenate([np.min([s[:dd] for s in sts], axis=0),
                        np.max([s[dd:] for s in sts], axis=0)])
    for c in ctxs:
        c.points_restat(g, n_total)


def _sharded(parts, unify=False):
    """begin -> per pass hist / host sum / select -> finish on one context per
    shard.  Returns (every context's medians, passes, modes)."""
    import _cdr

    ctxs = [_cdr.Context(0) for _ in parts]
    try:
        for c, X in zip(ctxs, parts):
            c.load_points(X)
        n_total = sum(X.shape[0] for X in parts)
        if unify:
            _unify(ctxs, n_total)
        modes = [c.info()["mode"] for c in ctxs]
        begun = [c.medians_global_begin(n_total) for c in ctxs]
        passes, words = begun[0]
        assert all(b == (passes, words) for b in begun) and words == parts[0].shape[1] * 512
        hists = [np.zeros(words, dtype=np.uint32) for _ in ctxs]
        for p in range(passes):
            for c, h in zip(ctxs, hists):
                c.medians_global_pass_hist(p, h)
            tot = np.sum(hists, axis=0, dtype=np.uint32)
            for c in ctxs:
                c.medians_global_pass_select(p, tot)
        return [c.medians_global_finish() for c in ctxs], passes, modes
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("name", ["three", "parity", "split", "empty"])
def test_sharded_passes(name, mode):
    """Shards of 5912 / 319 / 5 rows; two odd shards under an even total; the
    two middle values on different shards; a shard without rows (its storage
    mode is brought to the others' by points_restat, as a sharded run does)."""
    parts, exp = gc.split_middle_case(mode) if name == "split" else gc.shard_case(name, mode)
    meds, passes, modes = _sharded(parts, unify=(name == "empty"))
    assert passes == (4 if mode == "f32x" else 8) and modes == [MODE[mode]] * len(parts)
    for m in meds:
        _same(m, exp)


def test_sharded_passes_mixed_pair_unified():
    """An F32X shard next to an F64 one: after points_restat over both, both
    are F64, take 8 passes and give np.median of the union."""
    a, _ = gc.shard_case("parity", "f32x")
    b, _ = gc.shard_case("three", "f64")
    parts = [a[0], b[1]]
    meds, passes, modes = _sharded(parts, unify=True)
    assert modes == [mc.MODE_F64] * 2 and passes == 8
    for m in meds:
        _same(m, np.median(np.concatenate(parts), axis=0))


class _Exchange:
    """What two threads of one process need to all-reduce host arrays."""

    def __init__(self, world):
        self.bar = threading.Barrier(world, timeout=120)
        self.slots = [None] * world

    def reduce(self, rank, arr, fn):
        self.slots[rank] = np.array(arr)
        self.bar.wait()
        out = fn(np.stack(self.slots), axis=0)
        self.bar.wait()
        return out


class _ThreadComm:
    """cdr_dist.Comm's surface (a host communicator) over threads."""

    def __init__(self, ex, world, rank):
        self.world, self.rank, self.device, self.dist, self._ex = world, rank, None, self, ex

    def allreduce_i64(self, arr, op="sum"):
        fn = {"sum": np.sum, "min": np.min, "max": np.max}[op]
        return self._ex.reduce(self.rank, np.asarray(arr, dtype=np.int64), fn).astype(np.int64)

    def all_reduce(self, t):  # torch int32 tensor over the uint32 histogram
        import torch

        s = self._ex.reduce(self.rank, t.numpy().view(np.uint32), np.sum).astype(np.uint32)
        t.copy_(torch.from_numpy(s.view(np.int32)))


def _run_ranks(parts, fn):
    """fn(ctx, comm) on one thread and one context per shard; the results or
    the exceptions, in rank order."""
    import _cdr

    ex = _Exchange(len(parts))
    out = [None] * len(parts)

    def work(r):
        c = _cdr.Context(0)
        try:
            c.load_points(parts[r])
            out[r] = fn(c, _ThreadComm(ex, len(parts), r))
        except Exception as e:  # noqa: BLE001 - handed to the test
            out[r] = e
        finally:
            c.close()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(len(parts))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out


def test_sharded_global_medians_on_two_contexts():
    from cdr_dist import sharded_global_medians

    parts, exp = gc.split_middle_case("f64")
    for got in _run_ranks(parts, sharded_global_medians):
        assert not isinstance(got, Exception), got
        _same(got, exp)


def test_two_shards_left_in_different_modes():
    """One shard F32X, the other F64, not unified: every rank raises before
    the first pass and names unify_points."""
    from cdr_dist import sharded_global_medians

    a, _ = gc.shard_case("parity", "f32x")
    b, _ = gc.shard_case("parity", "f64")
    for got in _run_ranks([a[0], b[1]], sharded_global_medians):
        assert isinstance(got, RuntimeError) and "unify_points" in str(got), got


# ---- 7. scoring ----------------------------------------------------------------
def _tables(names):
    cats = ("Hot", "Shared", "Moderate", "Archival")
    w = {c: {nm: 0.5 + 0.1 * i for i, nm in enumerate(names)} for c in cats}
    dirs = {"Hot": {nm: 1 for nm in names}, "Shared": {nm: (1 if i % 2 else -1) for i, nm in enumerate(names)},
            "Moderate": {nm: 0 for nm in names}, "Archival": {nm: -1 for nm in names}}
    return w, dirs, {"Hot": 3, "Shared": 2, "Moderate": 1, "Archival": 4}


def test_scoring_global_medians_and_from_points(ctx):
    import kmeans_plusplus as kp
    import scoring

    X, exp = gc.case("minmax")
    names = ["f%d" % i for i in range(X.shape[1])]
    np.random.seed(0)
    kp.kmeans(X, 4, random_state=42, context=ctx)
    gm = scoring.global_medians(names, context=ctx)
    assert list(gm) == names and all(type(v) is np.float64 for v in gm.values())
    _same(np.array([gm[nm] for nm in names]), exp)
    with pytest.raises(ValueError, match="feature_names must name every column of X"):
        scoring.global_medians(names[:-1], context=ctx)
    w, dirs, rf = _tables(names)
    clf = scoring.ClusterClassifier.from_points(w, dirs, rf, names, context=ctx)
    assert clf.global_medians == gm
    ref = scoring.ClusterClassifier({nm: np.float64(v) for nm, v in zip(names, np.median(X, axis=0))},
                                    w, dirs, rf, context=ctx)
    got = clf.classify_labels(4, names)
    assert got == ref.classify_labels(4, names) and len(got) == 4
    # the placeholder medians the reference ships would not give the same deviations
    assert not np.allclose(exp, 0.5, atol=0.05)

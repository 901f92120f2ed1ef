"""The cluster medians (csrc/medians.hip) where grouping and radix select
change shape: more segments than workgroups, long segments, both middle
ranks parting at every key byte, counting-sort blocks and scan ranges, k past
the 256- and 1024-strides, every lane mapping of the histogram kernel, data
outside the unit cube, the product flow in both storage modes, sharded
passes over unequal shards, and the rules that invalidate grouped rows.

Every comparison is exact: np.testing.assert_array_equal against np.median
of the same rows (NaN positions included), plus the sign where a median can
be zero.  The labelled point sets come from tests/median_cases.py, whose
CPU test (tests/test_median_cases.py) checks that each is what it claims.
Preconditions a later change of a constant could hollow out (segments past
the grid cap, scan ranges, k past a stride, modes) are asserted next to the
case that needs them."""
import warnings

import numpy as np
import pytest

import data_families as df
import median_cases as mc

pytestmark = pytest.mark.gpu

SEG_GRID_CAP = 65536  # medians_segmented: grid = min(nseg, 65536)


def _np_medians(segs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.array([np.median(s) if len(s) else np.nan for s in segs])


def _run_segments(ctx, segs, lead=0):
    """medians_segmented over the list of arrays; `lead` unused values come
    first in the buffer, so offsets[0] == lead."""
    segs = [np.asarray(s, dtype=np.float64) for s in segs]
    offsets = np.full(len(segs) + 1, lead, dtype=np.int64)
    offsets[1:] += np.cumsum([s.size for s in segs])
    values = np.concatenate([np.full(lead, 1e300)] + segs)
    got = ctx.medians_segmented(values, offsets)
    exp = _np_medians(segs)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))
    return got


# ---- 2. the segmented kernel ----------------------------------------------
def test_segments_beyond_the_grid(ctx):
    """70 000 segments of 0-6 values on 65 536 workgroups: workgroups 0..4463
    take a second turn of the grid-stride loop, after a first segment that
    left by each of the loop's paths (NaN, empty, selected) and with even and
    odd sizes on either side."""
    nseg = 70_000
    assert nseg > SEG_GRID_CAP
    rng = np.random.default_rng(41)
    segs = [rng.normal(0, 3, int(m)) for m in rng.integers(0, 7, nseg)]
    nan, empty = np.array([1.0, np.nan, -2.0]), np.array([])
    for b in range(nseg - SEG_GRID_CAP):
        normal = rng.normal(0, 3, int(rng.integers(1, 7)))
        first, second = [(nan, normal), (empty, normal), (normal, nan), (normal, empty),
                         (rng.normal(0, 3, 4), rng.normal(0, 3, 5))][b % 5]
        segs[b], segs[b + SEG_GRID_CAP] = first, second
    got = _run_segments(ctx, segs)
    assert np.isnan(got[0]) and not np.isnan(got[SEG_GRID_CAP])       # (NaN, normal)
    assert not np.isnan(got[2]) and np.isnan(got[2 + SEG_GRID_CAP])   # (normal, NaN)


def test_segments_with_leading_offset(ctx):
    """offsets[0] != 0: the kernel sees offsets rebased to the copied range."""
    rng = np.random.default_rng(42)
    segs = [rng.normal(0, 1, int(m)) for m in rng.integers(0, 40, 300)]
    _run_segments(ctx, segs, lead=17)
    _run_segments(ctx, segs[:1], lead=5)


def test_long_segments(ctx):
    rng = np.random.default_rng(43)
    three = rng.choice(np.array([-1.5, 0.25, 7.0]), 300_001, p=[0.3, 0.4, 0.3])
    equal = np.full(70_001, -3.75)
    distinct = rng.permutation(np.arange(2 ** 16 + 1) * 0.5 - 1e4)
    assert np.unique(three).size == 3 and np.unique(distinct).size == 2 ** 16 + 1
    _run_segments(ctx, [three, equal, distinct, three[:300_000], distinct[:2 ** 16]])


def _bits_pair(p, rng):
    """Two doubles whose keys agree above byte p (0 = most significant) and
    differ in it; random bytes below."""
    sh = 8 * (7 - p)
    base = 0x4000000000000000  # 2.0: every planted pattern stays finite and positive
    lo = base | (1 << sh) | int(rng.integers(0, 1 << sh))
    hi = base | (2 << sh) | int(rng.integers(0, 1 << sh))
    v = np.array([lo, hi], dtype=np.uint64).view(np.float64)
    assert np.isfinite(v).all() and v[0] < v[1]
    return v


def test_segment_middles_part_at_each_byte(ctx):
    """Even-sized segments whose two middle values differ first in key byte p,
    p = 0..7 (the pass from which the two selections use separate histograms),
    for positive and for negative values, and one with equal middles."""
    rng = np.random.default_rng(44)
    segs = []
    for p in range(8):
        lo, hi = _bits_pair(p, rng)
        for sign in (1.0, -1.0):
            below = -np.abs(rng.normal(0, 1, 9)) - 1e306 if sign > 0 else -rng.random(9) - 1e308
            body = np.concatenate([below, sign * np.array([lo, hi]),
                                   np.full(9, np.inf) if sign > 0 else rng.random(9)])
            s = np.sort(body)
            assert sorted(s[9:11]) == sorted([sign * lo, sign * hi])
            segs.append(rng.permutation(body))
    segs.append(rng.permutation(np.concatenate([np.arange(9.0), [9.5, 9.5], 10 + np.arange(9.0)])))
    _run_segments(ctx, segs)


def test_segment_sign_and_range(ctx):
    tiny = 5e-324
    half = np.concatenate([-np.arange(1.0, 51.0), np.arange(1.0, 51.0)])
    segs = [[-np.inf, np.inf], [-np.inf, -np.inf], [np.inf], [tiny], [-tiny], [-tiny, tiny],
            [tiny, tiny], [tiny, 2 * tiny], [-tiny, -2 * tiny, -3 * tiny], half,
            np.concatenate([half, [-0.5, 0.25]]), [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [-0.0],
            [-0.0, 0.0, -0.0], [-1.0, -0.0, 0.0, 1.0], [-1.7976931348623157e308, 1.7976931348623157e308],
            [1.7976931348623157e308, 1.7976931348623157e308]]
    rng = np.random.default_rng(45)
    got = _run_segments(ctx, [rng.permutation(np.asarray(s, dtype=np.float64)) for s in segs])
    assert np.isnan(got[0])                          # NumPy's inf + -inf
    for i in (11, 12, 13, 14, 16):                   # the sum starts from +0.0
        assert got[i] == 0 and not np.signbit(got[i]), (i, got[i])


def test_segment_argument_errors(ctx):
    with pytest.raises(ValueError):
        ctx.medians_segmented(np.arange(6.0), np.array([0, 4, 2, 6]))
    with pytest.raises(ValueError):
        ctx.medians_segmented(np.arange(6.0), np.array([4, 2]))
    out = ctx.medians_segmented(np.arange(6.0), np.array([3]))
    assert out.shape == (0,) and out.dtype == np.float64


# ---- 3. label medians -------------------------------------------------------
def _step(ctx, C, mode):
    if mode == "f32x":
        ctx.lloyd_step(C)
    else:
        ctx.lloyd_step_f64(C)


def _check_case(ctx, name):
    """Load the case, step once from its anchors, require the designed
    labelling, compare all k x d medians."""
    X, C, lab, sizes = mc.case(name)
    mode = name.rsplit("-", 1)[1]
    k = sizes.size
    ctx.load_points(X)
    assert ctx.info()["mode"] == (mc.MODE_F32X if mode == "f32x" else mc.MODE_F64), ctx.info()
    _step(ctx, C, mode)
    got_lab = ctx.labels()
    np.testing.assert_array_equal(np.bincount(got_lab, minlength=k), sizes)
    np.testing.assert_array_equal(got_lab, lab)
    got = ctx.medians_by_label(k)
    exp = mc.ref_medians(X, lab, k)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))
    return X, lab, sizes, got


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("n", mc.BLOCK_N)
def test_label_medians_blocks_and_ranges(ctx, n, mode):
    """d = 2, k = 7 at the edges of the counting-sort block (4096 points) and
    of the column-scan range (64 blocks): one block short, full, one point
    over; one range full, one block over (rbase != 0), three ranges."""
    nblk = -(-n // mc.MG_BLOCK)
    nr = -(-nblk // mc.MG_RANGE)
    want = {4095: (1, 1), 4096: (1, 1), 4097: (2, 1), 262_144: (64, 1), 262_145: (65, 2),
            528_385: (130, 3)}
    assert (nblk, nr) == want[n]
    X, lab, sizes, _ = _check_case(ctx, "blocks-%d-%s" % (n, mode))
    # every cluster has rows in every block, so each block offset carries weight
    if n >= mc.MG_BLOCK:
        per_block = np.stack([np.bincount(lab[b * mc.MG_BLOCK:(b + 1) * mc.MG_BLOCK], minlength=7)
                              for b in range(n // mc.MG_BLOCK)])
        assert per_block.min() >= 1


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("k,d", mc.BIG_K)
def test_label_medians_k_beyond_the_strides(ctx, k, d, mode):
    """k past the 256-thread stride of mg_count / mg_scatter / the scans
    (257), past mg_scan_b's 1024 (1025: its carry), k = 1500 at d = 17 (a
    shape of the large-k Lloyd path) and past two strides (2049).  Every
    cluster is non-empty, so the bases of clusters >= 1024 carry weight."""
    X, lab, sizes, got = _check_case(ctx, "bigk-%d-%d-%s" % (k, d, mode))
    assert sizes.min() >= 1 and not np.isnan(got).any()
    if k > 1024:
        assert np.bincount(lab, minlength=k)[1024:].min() >= 1
        assert X.shape[0] > mc.MG_BLOCK  # more than one block under the large k


def test_label_medians_k_limits(ctx):
    X, C, lab, sizes = mc.case("lanes-5-f32x")
    ctx.load_points(X)
    ctx.lloyd_step(C)
    k = sizes.size
    assert mc.MG_MAXK == 8192
    with pytest.raises(NotImplementedError):
        ctx.medians_by_label(mc.MG_MAXK + 1)
    with pytest.raises(ValueError):
        ctx.medians_by_label(k - 1)
    # k above the labels' k is allowed: the extra clusters are empty
    got = ctx.medians_by_label(k + 3)
    np.testing.assert_array_equal(got, mc.ref_medians(X, lab, k + 3))
    assert np.isnan(got[k:]).all()


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("d", mc.LANE_D)
def test_label_medians_lane_mapping(ctx, d, mode):
    """mg_hist / mg_scatter spread lanes over (row, feature) by D2 = the next
    power of two >= min(d, 64): R = 16 (64 / D2) rows per step, 8 R per
    unrolled turn.  Cluster sizes 1, 2, R-1, R, R+1, 8R+1 sit on both loop
    boundaries of every d; d = 65, 127, 128 add the second feature chunk."""
    R = mc.hist_rows(d)
    D2 = 64 * mc.MG_WAVES // R
    assert D2 >= min(d, 64) > D2 // 2 or d == 1
    X, lab, sizes, _ = _check_case(ctx, "lanes-%d-%s" % (d, mode))
    assert tuple(sizes) == (1, 2, R - 1, R, R + 1, mc.MG_U * R + 1)


@pytest.mark.parametrize("mode", mc.MODES)
def test_label_medians_where_the_ranks_part(ctx, mode):
    """d = 8, k = 5 with planted columns: middle values equal, neighbours,
    of opposite sign, differing first in each byte the key has (4 in F32X, 8
    in F64), tie runs through both middle ranks, and a column of -0.0 / +0.0
    only, whose median is +0.0."""
    X, lab, sizes, got = _check_case(ctx, "part-" + mode)
    notes = {(j, f): note for j, f, _, note in mc.part_plants(mode, 11)}
    assert sum(n.startswith("byte") for n in notes.values()) == (4 if mode == "f32x" else 8)
    for (j, f), note in notes.items():
        if note in ("zeros", "signed zeros in the middle"):
            assert got[j, f] == 0 and not np.signbit(got[j, f]), (j, f, got[j, f])
    assert got[0, 1] == 0.0 and got[0, 0] == 0.125 and got[1, 7] == 4.5 and got[2, 0] == 8.25


@pytest.mark.parametrize("name", df.FAMILIES)
def test_label_medians_data_families(ctx, name):
    """Every family of tests/data_families.py at 24 001 x 16, k = 64: offsets
    with 24 significant bits, 2^-126-scaled floats, signed whole numbers,
    constant columns, doubles up to 2^50."""
    case = (name,) + df.SHAPES_ALL
    n, d, k = df.SHAPES_ALL
    X = df.data(case)
    ctx.load_points(X)
    info = ctx.info()
    if df.EXPECT[name] is not None:
        assert info["mode"] == df.EXPECT[name][0], info
    rng = np.random.default_rng(900 + df.FAMILIES.index(name))
    C = X[rng.choice(n, k, replace=False)].copy()
    _step(ctx, C, "f32x" if info["mode"] == mc.MODE_F32X else "f64")
    lab = ctx.labels()
    assert lab.min() >= 0 and lab.max() < k
    got = ctx.medians_by_label(k)
    exp = mc.ref_medians(X, lab, k)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))


def _classifier(ctx, names):
    from scoring import ClusterClassifier

    gm = {nm: 0.5 for nm in names}
    w = {c: {nm: 1.0 for nm in names} for c in ("Hot", "Shared", "Moderate", "Archival")}
    dirs = {"Hot": {nm: 1 for nm in names}, "Shared": {nm: 1 for nm in names},
            "Moderate": {nm: 0 for nm in names}, "Archival": {nm: -1 for nm in names}}
    rf = {"Hot": 3, "Shared": 2, "Moderate": 1, "Archival": 4}
    return ClusterClassifier(gm, w, dirs, rf, context=ctx)


def _check_product_flow(ctx, X, lab, k):
    """What main.py does after kmeans(): medians by the returned labels, and
    classify_labels against classify on the lists main.py builds."""
    d = X.shape[1]
    got = ctx.medians_by_label(k)
    np.testing.assert_array_equal(got, mc.ref_medians(X, lab, k))
    names = ["f%d" % i for i in range(d)]
    clf = _classifier(ctx, names)
    lists = {"C%d" % j: {nm: X[lab == j, i].tolist() for i, nm in enumerate(names)}
             for j in range(k)}
    assert clf.classify_labels(k, names) == clf.classify(lists)


def test_product_flow_f64(ctx):
    """kmeans() on min-max doubles (F64 storage, the device run), then the
    label medians and classify_labels."""
    import kmeans_plusplus as kp
    from test_gpu_f64_update import _minmax

    X = _minmax(np.random.default_rng(46), 30_000, 5)
    np.random.seed(0)
    _, lab = kp.kmeans(X, 4, random_state=42, context=ctx)
    assert ctx.info()["mode"] == mc.MODE_F64
    assert np.bincount(lab, minlength=4).min() >= 1
    _check_product_flow(ctx, X, lab, 4)


def test_product_flow_f32x_bounded_screen(ctx):
    """The same after kmeans() on 2^-24 grid data, with enough steps for the
    device loop to end in the bounded screen (its labels are the ones the
    medians group by)."""
    import kmeans_plusplus as kp
    from test_gpu_loop import _grid_uniform

    X = _grid_uniform(24_539, 7, 47)
    np.random.seed(0)
    _, lab = kp.kmeans(X, 20, random_state=42, max_iter=8, context=ctx)
    assert ctx.info()["mode"] == mc.MODE_F32X
    assert ctx.profile_kernel().startswith("screen32b"), ctx.profile_kernel()
    np.testing.assert_array_equal(ctx.labels(), lab)
    _check_product_flow(ctx, X, lab, 20)


# ---- 4. sharded passes, several contexts in one process ----------------------
def _shard_rows(lab, counts, seed):
    """Row indices per shard: shard s takes counts[s][j] rows of cluster j."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    rows = [[] for _ in counts]
    for j in range(counts.shape[1]):
        idx = rng.permutation(np.flatnonzero(lab == j))
        assert idx.size == counts[:, j].sum(), (j, idx.size)
        cut = np.concatenate([[0], np.cumsum(counts[:, j])])
        for s in range(counts.shape[0]):
            rows[s].append(idx[cut[s]:cut[s + 1]])
    return [rng.permutation(np.concatenate(r)) for r in rows]


def _sharded_medians(parts, C, k, mode, unify=False):
    """The pass API on one context per shard, the all-reduces done on the
    host: group -> summed counts -> begin -> per pass hist / sum / select ->
    finish.  Returns (medians of every context, passes, modes)."""
    import _cdr

    ctxs = [_cdr.Context(0) for _ in parts]
    try:
        for c, (X, _) in zip(ctxs, parts):
            c.load_points(X)
        if unify:  # cdr_dist.unify_points with the MIN / MAX all-reduce done here
            sts = [c.points_stats() for c in ctxs]
            dd = (sts[0].size - 3) // 2
            g = np.concatenate([np.min([s[:dd] for s in sts], axis=0),
                                np.max([s[dd:] for s in sts], axis=0)])
            for c in ctxs:
                c.points_restat(g, sum(X.shape[0] for X, _ in parts))
        modes = [c.info()["mode"] for c in ctxs]
        for c, (_, lab) in zip(ctxs, parts):
            _step(c, C, mode)
            np.testing.assert_array_equal(c.labels(), lab)
        local = [c.medians_group(k) for c in ctxs]
        for cnt, (_, lab) in zip(local, parts):
            np.testing.assert_array_equal(cnt, np.bincount(lab, minlength=k))
        total = np.sum(local, axis=0)
        begun = [c.medians_begin(total) for c in ctxs]
        passes, words = begun[0]
        assert all(b == (passes, words) for b in begun) and words == k * C.shape[1] * 512
        hists = [np.zeros(words, dtype=np.uint32) for _ in ctxs]
        for p in range(passes):
            for c, h in zip(ctxs, hists):
                c.medians_pass_hist(p, h)
            tot = np.sum(hists, axis=0, dtype=np.uint32)
            for c in ctxs:
                c.medians_pass_select(p, tot)
        return [c.medians_finish() for c in ctxs], passes, modes
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("counts", [mc.TWO_SHARDS, mc.THREE_SHARDS], ids=["two", "three"])
def test_sharded_passes_uneven_shards(mode, counts):
    """Clusters that live on one shard only (2 and 4 on shard 0, 3 on shard
    1), an empty cluster, local counts even / odd / 0 against a global count
    of the other parity (40 + 61 = 101, 51 + 49 = 100, 7 + 0); three shards of
    5912, 319 and 5 rows."""
    counts = np.asarray(counts)
    sizes = counts.sum(axis=0)
    k, d = sizes.size, 3
    if counts.shape[0] == 2:
        assert (counts[0, 0] % 2, counts[1, 0] % 2, sizes[0] % 2) == (0, 1, 1)
        assert (counts[0, 1] % 2, counts[1, 1] % 2, sizes[1] % 2) == (1, 1, 0)
        assert counts[1, 2] == 0 and sizes[2] % 2 == 1
        assert (counts[1] == 0).sum() >= 3 and counts[0, 3] == 0 and sizes[5] == 0
    else:
        assert counts.sum(axis=1).max() > 1000 * counts.sum(axis=1).min()
    X, C, lab, designed = mc.case("shards%d-%s" % (counts.shape[0], mode))
    np.testing.assert_array_equal(designed, sizes)
    rows = _shard_rows(lab, counts, 51)
    meds, passes, modes = _sharded_medians([(X[r], lab[r]) for r in rows], C, k, mode)
    assert passes == (4 if mode == "f32x" else 8)
    assert modes == [mc.MODE_F32X if mode == "f32x" else mc.MODE_F64] * len(rows)
    exp = mc.ref_medians(X, lab, k)
    assert np.isnan(exp[sizes == 0]).all() and not np.isnan(exp[sizes > 0]).any()
    for m in meds:
        np.testing.assert_array_equal(m, exp)


def test_sharded_passes_mixed_pair_unified():
    """Shard 0 holds grid data, shard 1 one double that no float32 holds:
    alone they are F32X and F64; after points_stats / points_restat over both
    (cdr_dist.unify_points) both are F64, take 8 passes, and the medians are
    those of the whole set."""
    import _cdr

    X, C, lab, sizes = mc.case("mixed-f32x")
    k = sizes.size
    X = X.copy()
    rows = _shard_rows(lab, [sizes // 2, sizes - sizes // 2], 53)
    i = rows[1][5]
    X[i, 2] += np.pi * 2.0 ** -20
    assert np.float64(np.float32(X[i, 2])) != X[i, 2] and abs(X[i, 2] - C[lab[i], 2]) < 1
    alone = []
    for r in rows:
        c = _cdr.Context(0)
        try:
            c.load_points(X[r])
            alone.append(c.info()["mode"])
        finally:
            c.close()
    assert alone == [mc.MODE_F32X, mc.MODE_F64]
    meds, passes, modes = _sharded_medians([(X[r], lab[r]) for r in rows], C, k, "f64",
                                           unify=True)
    assert modes == [mc.MODE_F64, mc.MODE_F64] and passes == 8
    exp = mc.ref_medians(X, lab, k)
    for m in meds:
        np.testing.assert_array_equal(m, exp)


# ---- 5. grouped rows do not outlive what they were built from ----------------
def test_grouped_rows_end_with_new_points(ctx):
    """group, then load_points of other data of the same shape and mode:
    medians_begin must refuse (it would return the old points' medians)."""
    X, C, lab, _ = mc.case("stale_a-f32x")
    X2, _, lab2, _ = mc.case("stale_b-f32x")
    assert X.shape == X2.shape and not np.array_equal(X, X2)
    ctx.load_points(X)
    ctx.lloyd_step(C)
    counts = ctx.medians_group(3)
    ctx.load_points(X2)
    assert ctx.info()["mode"] == mc.MODE_F32X
    with pytest.raises(RuntimeError, match="cdr_medians_group"):
        ctx.medians_begin(counts)
    # and the normal order still works on the new points
    ctx.lloyd_step(C)
    np.testing.assert_array_equal(ctx.medians_by_label(3), mc.ref_medians(X2, lab2, 3))


def test_grouped_rows_end_with_new_labels(ctx):
    """group, then another Lloyd step with other centroids: the rows are
    grouped by labels that no longer exist."""
    X, C, lab, _ = mc.case("stale_a-f64")
    ctx.load_points(X)
    ctx.lloyd_step_f64(C)
    counts = ctx.medians_group(3)
    ctx.lloyd_step_f64(C[::-1].copy())
    np.testing.assert_array_equal(ctx.labels(), 2 - lab)
    with pytest.raises(RuntimeError, match="cdr_medians_group"):
        ctx.medians_begin(counts)
    # the same once the passes have begun: no pass or finish on the old rows
    counts = ctx.medians_group(3)
    passes, words = ctx.medians_begin(counts)
    ctx.lloyd_step_f64(C)
    hist = np.zeros(words, dtype=np.uint32)
    for call in (lambda: ctx.medians_pass_hist(0, hist), lambda: ctx.medians_pass_select(0, hist),
                 ctx.medians_finish):
        with pytest.raises(RuntimeError, match="cdr_medians_group"):
            call()
    ctx.lloyd_step_f64(C[::-1].copy())
    np.testing.assert_array_equal(ctx.medians_by_label(3), mc.ref_medians(X, 2 - lab, 3))

"""GPU parity of seeding + Lloyd (libcdr via the drop-in module) against the
reference golden vectors and the pinned oracle."""
import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import kmeans_oracle as ko
from oracle import synth

pytestmark = pytest.mark.gpu


def _cases():
    with open(os.path.join(GOLDEN, "kmeans_cases.json")) as fh:
        meta = json.load(fh)
    arrays = np.load(os.path.join(GOLDEN, "kmeans_cases.npz"))
    out = []
    for i, m in enumerate(meta["cases"]):
        X = synth.generate(*m["gen"]) if "gen" in m else arrays[f"c{i}_X"]
        get = lambda key: arrays[f"c{i}_{key}"] if f"c{i}_{key}" in arrays else None  # noqa
        out.append((m, X, get("init"), get("centroids"), get("labels")))
    return out


CASES = _cases()


def test_generator_bit_identical_to_numpy_mirror(ctx):
    ctx.generate_points(100000, 12345, 30000, 16, 64, 0x5EED)
    got = ctx.get_rows(np.arange(0, 30000, 7))
    exp = synth.generate(100000, 12345, 30000, 16, 64, 0x5EED)[::7]
    np.testing.assert_array_equal(got, exp)
    inf = ctx.info()
    assert inf["mode"] == 1 and inf["scale_bits"] <= 24


@pytest.mark.parametrize("case", CASES, ids=[c[0]["name"] for c in CASES])
def test_seeding_and_lloyd_match_reference(ctx, case):
    import kmeans_plusplus as kp

    m, X, init, C, labels = case
    if m.get("error"):
        with pytest.raises(ValueError, match="Probabilities contain NaN"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                kp.kmeans_plusplus_init(X, m["k"], random_state=m["rs"], context=ctx)
        return
    got_init = kp.kmeans_plusplus_init(X, m["k"], random_state=m["rs"], context=ctx)
    np.testing.assert_array_equal(got_init, init)
    if m["seed_only"]:
        return
    np.random.seed(m["np_seed"])
    got_C, got_l = kp.kmeans(X, m["k"], number_of_files=X.shape[0], random_state=m["rs"],
                             context=ctx)
    assert got_l.dtype == np.int64
    np.testing.assert_array_equal(got_l, labels)  # ARI = 1.0, bit-identical
    np.testing.assert_array_equal(got_C, C)


def test_n_above_10000_raises_reference_typeerror(ctx):
    import kmeans_plusplus as kp

    X = synth.generate(10001, 0, 10001, 2, 3, 1)
    with pytest.raises(TypeError, match="cannot be interpreted as an integer"):
        kp.kmeans(X, 3, number_of_files=10001, random_state=0, context=ctx)


def test_lloyd_partials_exact_vs_oracle(ctx):
    n, d, k = 300000, 16, 64
    X = synth.generate(n, 0, n, d, k, 77)
    ctx.load_points(X)
    assert ctx.info()["mode"] == 1
    rng = np.random.default_rng(0)
    C = X[rng.choice(n, k, replace=False)] + rng.normal(0, 1e-3, (k, d))
    out = ctx.lloyd_step(C)
    labels, exp = ko.lloyd_partials(X, C, ctx.info()["scale_bits"])
    np.testing.assert_array_equal(ctx.labels(), labels)
    np.testing.assert_array_equal(out, exp)
    fb = ctx.fallback_count()
    assert 0 <= fb < n // 20, fb


def test_screen_error_within_certified_bound(ctx):
    n, d, k = 20000, 16, 64
    X = synth.generate(n, 0, n, d, k, 5)
    ctx.load_points(X)
    rng = np.random.default_rng(1)
    C = X[rng.choice(n, k, replace=False)]
    T, thr = ctx.debug_screen(C)
    # recompute Q_j = ||xhat - chat_j||^2 in fp64 with the same transform
    mu = np.float32(0.5 * (X.min(axis=0) + X.max(axis=0))).astype(np.float64)
    dev = max((X.max(axis=0) - mu).max(), (mu - X.min(axis=0)).max())
    sig = -np.frexp(dev)[1]
    xh = (X - mu) * 2.0 ** sig
    ch = (C - mu) * 2.0 ** sig
    Q = ((xh[:, None, :] - ch[None, :, :]) ** 2).sum(axis=2)
    xx = (xh ** 2).sum(axis=1)
    diff = T.astype(np.float64) - Q  # = eps shift + error; eps common to all j
    spread = diff.max(axis=1) - diff.min(axis=1)
    bound = thr[0] + thr[1] * xx  # certification threshold covers 2x the error
    assert np.all(spread <= bound), float((spread / bound).max())


def test_two_shards_equal_one_shard(ctx):
    import _cdr

    n, d, k = 3 * 8192 + 500, 8, 16
    X = synth.generate(n, 0, n, d, k, 3)
    C = X[:k] + 1e-4
    ctx.load_points(X)
    full = ctx.lloyd_step(C)
    lab = ctx.labels()
    b = _cdr.Context(ctx.device)
    try:
        cut = 2 * 8192
        ctx.load_points(X[:cut])
        b.load_points(X[cut:])
        a1 = ctx.lloyd_step(C)
        a2 = b.lloyd_step(C)
        np.testing.assert_array_equal(a1 + a2, full)
        np.testing.assert_array_equal(np.concatenate([ctx.labels(), b.labels()]), lab)
        # seeding scan chained over the two shards == single shard
        ctx.load_points(X)
        ctx.seed_reset()
        ctx.seed_update(X[5])
        tot = _cdr.host_seq_sum(ctx.seed_block_sums())
        c_full = ctx.seed_scan(tot, 0.0)
        idx_full = ctx.seed_search(c_full, 0.6180339887)
        ctx.load_points(X[:cut])
        ctx.seed_reset()
        ctx.seed_update(X[5])
        b.seed_reset()
        b.seed_update(X[5])
        bs = np.concatenate([ctx.seed_block_sums(), b.seed_block_sums()])
        assert _cdr.host_seq_sum(bs) == tot
        c1 = ctx.seed_scan(tot, 0.0)
        c2 = b.seed_scan(tot, c1)
        assert c2 == c_full
        i1, i2 = ctx.seed_search(c2, 0.6180339887), b.seed_search(c2, 0.6180339887)
        got = i1 if i1 >= 0 else cut + i2
        assert got == idx_full
        probs = ko.sqdist_rows(X, X[5])
        probs = np.sqrt(probs) ** 2
        probs = probs / probs.sum()
        cdf = np.cumsum(probs)
        cdf /= cdf[-1]
        assert cdf[-1] == 1.0
        assert np.cumsum(probs)[-1] == c_full
        assert idx_full == np.searchsorted(cdf, 0.6180339887, side="right")
    finally:
        b.close()


@pytest.mark.parametrize("n,d,k", [(200000, 16, 64), (120000, 5, 4), (60000, 64, 16),
                                   (50000, 3, 100), (40000, 24, 33)])
def test_seeding_and_steps_vs_oracle_large(ctx, n, d, k):
    """Beyond the reference's n <= 10000 limit: oracle (pinned) as the checker."""
    import kmeans_plusplus as kp

    X = synth.generate(n, 0, n, d, max(k, 2), n + d)
    init = kp.kmeans_plusplus_init(X, k, random_state=42, context=ctx)
    np.testing.assert_array_equal(init, ko.kmeans_plusplus_init(X, k, random_state=42))
    np.random.seed(0)
    C, lab = kp.kmeans(X, k, random_state=42, max_iter=3, context=ctx)
    np.random.seed(0)
    C2, lab2 = ko.kmeans(X, k, random_state=42, max_iter=3)
    np.testing.assert_array_equal(lab, lab2)
    np.testing.assert_array_equal(C, C2)


def test_full_size_properties_config2(ctx):
    """BASELINE config 2 size (10M x 8, k=16): size-independent invariants."""
    n, d, k = 10_000_000, 8, 16
    ctx.generate_points(n, 0, n, d, k, 0x5EED)
    rng = np.random.default_rng(2)
    C = ctx.get_rows(rng.choice(n, k, replace=False))
    out = ctx.lloyd_step(C)
    lab = ctx.labels()
    assert out[:, d].sum() == n
    np.testing.assert_array_equal(np.bincount(lab, minlength=k), out[:, d])
    # labels of a random sample agree with the exact oracle
    sample = np.sort(rng.choice(n, 20000, replace=False))
    Xs = ctx.get_rows(sample)
    np.testing.assert_array_equal(lab[sample], ko.assign(Xs, C))
    # the int64 sums of one whole cluster recomputed on the host from its rows
    # (the points are multiples of 2^-S: exact)
    S = ctx.info()["scale_bits"]
    j = int(np.argmax(out[:, d]))
    idx = np.flatnonzero(lab == j)
    assert idx.size == out[j, d] > 0
    rows = ctx.get_rows(idx)
    np.testing.assert_array_equal(np.ldexp(rows, S).astype(np.int64).sum(axis=0), out[j, :d])
    assert ctx.fallback_count() < n // 50


@pytest.mark.parametrize("n,d,k", [(150000, 16, 64), (70000, 8, 16), (30000, 5, 40),
                                   (20000, 12, 7)])
def test_incremental_update_equals_full_recompute(ctx, n, d, k, monkeypatch):
    """screen32 keeps exact int64 running sums and applies only the changes of
    points that switched cluster; every step must equal a from-scratch step
    (and the oracle), including steps where clusters empty out."""
    X = synth.generate(n, 0, n, d, max(k, 2), 1000 + n + d)
    ctx.load_points(X)
    S = ctx.info()["scale_bits"]
    rng = np.random.default_rng(d)
    C = X[rng.choice(n, k, replace=False)].copy()
    C[-1] = 7.0  # far away: an empty cluster from the first step on
    for step in range(5):
        out = ctx.lloyd_step(C)
        lab = ctx.labels()
        exp_lab, exp = ko.lloyd_partials(X, C, S)
        np.testing.assert_array_equal(lab, exp_lab)
        np.testing.assert_array_equal(out, exp)
        # same step from scratch (full update) on a second context
        monkeypatch.setenv("CDR_NO_DELTA", "1")
        import _cdr
        b = _cdr.Context(ctx.device)
        try:
            b.load_points(X)
            np.testing.assert_array_equal(b.lloyd_step(C), out)
        finally:
            b.close()
            monkeypatch.delenv("CDR_NO_DELTA")
        cnt = out[:, d]
        means = np.ldexp(out[:, :d].astype(np.float64), -S) / np.maximum(cnt, 1)[:, None]
        C = np.where(cnt[:, None] > 0, means, C)
        if step == 2:  # reseed the empty cluster onto a point, as the reference does
            C[-1] = X[12345 % n]


@pytest.mark.parametrize("d", [16, 11, 8, 5])
def test_hi_only_screen_near_ties(ctx, d):
    """The DELTA steps screen fp16(xhat) alone (screen32p's drains): points put
    on the bisectors of centroid pairs and a few fp16 ulps off them must still
    get the reference's label (the per-point certificate sends them to the
    exact fallback)."""
    n, k = 200000, 64
    X = synth.generate(n, 0, n, d, k, 4242 + d).copy()
    rng = np.random.default_rng(d)
    C2 = X[rng.choice(n, k, replace=False)].astype(np.float64)
    m = n // 4  # a quarter of the points: near-ties of the second step's centroids
    a = rng.integers(0, k, m)
    b = (a + 1 + rng.integers(0, k - 1, m)) % k
    eps = rng.choice([0.0, 2.0 ** -11, -2.0 ** -11, 2.0 ** -13, -2.0 ** -13, 2.0 ** -20], m)
    P = 0.5 * (C2[a] + C2[b]) + eps[:, None] * (C2[b] - C2[a])
    P = np.clip(np.round(P * 2.0 ** 24) * 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24)
    X[:m] = P.astype(np.float32)
    ctx.load_points(X)
    assert ctx.info()["mode"] == 1
    S = ctx.info()["scale_bits"]
    C1 = C2 + rng.normal(0, 1e-3, C2.shape)
    for step, C in enumerate((C1, C2, C2)):
        out = ctx.lloyd_step(C)
        exp_lab, exp = ko.lloyd_partials(X, C, S)
        np.testing.assert_array_equal(ctx.labels(), exp_lab, err_msg=f"step {step}")
        np.testing.assert_array_equal(out, exp, err_msg=f"step {step}")
        if step == 1:  # the near-ties went to the exact fallback
            assert ctx.fallback_count() > m // 10, ctx.fallback_count()


@pytest.mark.parametrize("n,outlier", [(3_000_001, False), (1_200_000, True), (9_000_001, False)])
def test_seeding_many_blocks_vs_oracle(ctx, n, outlier):
    """Seeding over hundreds of 8192-blocks: the block-transfer walk crosses
    binades between blocks and inside them, and the 64-ary block search runs
    several rounds.  The outlier case makes one D^2 dominate (tiny
    probabilities everywhere else, many crossings in the first blocks).  9M
    rows: 1099 block sums, so the device total runs over two staged chunks
    of 1024, the second one partial."""
    import kmeans_plusplus as kp

    X = synth.generate(n, 0, n, 16, 8, 77 + n)
    if outlier:
        X[n // 3] = 64.0
    init = kp.kmeans_plusplus_init(X, 8, random_state=7, context=ctx)
    np.testing.assert_array_equal(init, ko.kmeans_plusplus_init(X, 8, random_state=7))


# (n, d, family): every arm of the update's dispatcher (csrc/seed_update.hip
# seed_update) at its smallest interesting shape — the compacted fp16 kernel
# (d = 8, 16), the wide fp16 kernel (d = 32, 64; a one-row tail block, and a
# single partial block: no full block at all), the plain kernel unrolled (d =
# 5) and by runtime d (d = 20), and the fp64 kernel of F64 mode.
_SEED_SUM_CASES = [(8192 * 37 + 1234, 16, "synth"), (8192 * 5, 5, "synth"), (5000, 16, "synth"),
                   (8192 * 3 + 1, 20, "synth"), (8192 * 2 + 77, 8, "synth"),
                   (8192 * 2 + 77, 32, "synth"), (8192 + 1, 64, "synth"), (3000, 64, "synth"),
                   (8192 * 2 + 5, 5, "raw_f64")]


@pytest.mark.parametrize(
    "n,d,fam", _SEED_SUM_CASES,
    ids=["%d-%d%s" % (n, d, "" if fam == "synth" else "-" + fam) for n, d, fam in _SEED_SUM_CASES])
def test_seed_block_sums_and_scan_exact(ctx, n, d, fam):
    """Per-block D^2 sums are NumPy's pairwise add.reduce of each 8192 chunk,
    the total is dist_sq.sum(), and the device scan's last running value is
    np.cumsum(dist_sq / total)[-1] — all bit-exact (kmeans_plusplus.py:14-19)."""
    import _cdr
    import data_families as df

    if fam == "synth":
        X = synth.generate(n, 0, n, d, 8, 1000 + n + d)
    else:
        X = df.family(fam, n, d, 1000 + n + d)
    ctx.load_points(X)
    assert ctx.info()["mode"] == (df.MODE_F64 if fam == "raw_f64" else df.MODE_F32X)
    ctx.seed_reset()
    dist = np.full(n, np.inf)
    for c in (X[3], X[n // 2], X[n - 1]):
        ctx.seed_update(c)
        dist = np.minimum(dist, np.sqrt(ko.sqdist_rows(X, c)) ** 2)
        bs = ctx.seed_block_sums()
        want = np.array([np.add.reduce(dist[i:i + 8192]) for i in range(0, n, 8192)])
        np.testing.assert_array_equal(bs, want)
        total = _cdr.host_seq_sum(bs)
        assert total == dist.sum()
        assert ctx.seed_scan(total, 0.0) == np.cumsum(dist / total)[-1]


@pytest.mark.parametrize("n,d,k", [(20000, 64, 1024), (30000, 24, 300), (25000, 40, 700),
                                   (12000, 64, 129)])
def test_large_k_path_vs_oracle(ctx, n, d, k):
    """Config-5 regime (k*(d+1) beyond a workgroup's LDS): screen_big L1
    one-product MFMA screen, L2 three-product re-screen, L3 exact fp64, and the
    feature-pass update — labels and centroids bit-identical to the oracle."""
    import kmeans_plusplus as kp

    X = synth.generate(n, 0, n, d, k, 7 * n + d)
    rng = np.random.default_rng(k)
    C0 = X[np.sort(rng.choice(n, k, replace=False))]
    ctx.load_points(X)
    out = ctx.lloyd_step(C0)
    assert ctx.profile_kernel().startswith("screen_big"), ctx.profile_kernel()
    want_labels, want = ko.lloyd_partials(X, C0, ctx.info()["scale_bits"])
    np.testing.assert_array_equal(ctx.labels(), want_labels)
    np.testing.assert_array_equal(out, want)
    np.random.seed(0)
    C, lab = kp.kmeans(X, k, random_state=42, max_iter=2, context=ctx)
    np.random.seed(0)
    C2, lab2 = ko.kmeans(X, k, random_state=42, max_iter=2)
    np.testing.assert_array_equal(lab, lab2)
    np.testing.assert_array_equal(C, C2)


@pytest.mark.parametrize("n,d,k", [(50, 64, 300), (1000, 33, 257), (4097, 17, 1500)])
def test_large_k_ragged_shapes(ctx, n, d, k):
    """screen_big edge shapes: fewer points than centroids, d not a multiple
    of 16, k not a multiple of 32 (padding rows and feature slots)."""
    X = synth.generate(n, 0, n, d, min(k, 64), 11 * n + d)
    rng = np.random.default_rng(n)
    C0 = X[rng.integers(0, n, k)] + 0.0
    C0[::7] += 2.0 ** -20  # centroids off the data points, still on a fine grid
    ctx.load_points(X)
    out = ctx.lloyd_step(C0)
    assert ctx.profile_kernel().startswith("screen_big"), ctx.profile_kernel()
    want_labels, want = ko.lloyd_partials(X, C0, ctx.info()["scale_bits"])
    np.testing.assert_array_equal(ctx.labels(), want_labels)
    np.testing.assert_array_equal(out, want)


def test_f32x_gate_keeps_numpy_mean_exact(ctx):
    """F32X (exact int64 sums) only while every cluster partial sum stays below
    2^53 grid units: absmax * 2^S * n < 2^53, else F64 mode."""
    v = float(2 ** 29 - 32)  # fp32-exact, integer grid (S = 0), |x| 2^S < 2^30
    for n, want in ((2 ** 23, 1), (2 ** 24 + 8, 2)):
        X = np.full((n, 1), v)
        X[::3] = 1.0
        ctx.load_points(X)
        inf = ctx.info()
        assert inf["mode"] == want, (n, inf)


@pytest.mark.parametrize("n,outlier", [(8192 * 40 + 77, False), (8192 * 25, True), (3000, False)])
def test_seed_program_cend_exact(ctx, n, outlier):
    """The program scan (csrc/seed_scan.hip seg_* kernels) fills the per-block
    running values that seed_search reads: searchsorted(cumsum / c_last, u,
    'right') for u exactly at block ends and at random points equals NumPy's
    (kmeans_plusplus.py:19)."""
    import _cdr

    X = synth.generate(n, 0, n, 16, 8, 4242 + n)
    if outlier:
        X[n // 2] = 50.0
    ctx.load_points(X)
    ctx.seed_reset()
    st0 = ctx.seed_stats()
    dist = np.full(n, np.inf)
    for c in (X[1], X[n // 3]):
        ctx.seed_update(c)
        dist = np.minimum(dist, np.sqrt(ko.sqdist_rows(X, c)) ** 2)
        total = _cdr.host_seq_sum(ctx.seed_block_sums())
        cum = np.cumsum(dist / total)
        c_last = ctx.seed_scan(total, 0.0)
        assert c_last == cum[-1]
        cdf = cum / c_last
        us = [cdf[i] for i in range(8191, n - 1, 8192)] + list(np.random.default_rng(n).random(20))
        for u in us:
            want = int(np.searchsorted(cdf, u, side="right"))
            got = ctx.seed_search(c_last, float(u))
            assert got == (want if want < n else -1), (u, got, want)
    st = ctx.seed_stats()
    assert st["programs"] - st0["programs"] == 2  # both scans went through programs
    assert st["fallbacks"] == st0["fallbacks"]    # and no guess failed


def test_seed_programs_compose_over_shards(ctx):
    """Sharded seeding without the rank chain: the second shard's program,
    built from a guessed start, composed on the host from the first shard's
    exact carry (cdr_seed_program_eval) = its exact scan (cdr_seed_scan_end)
    = the single-shard scan."""
    import _cdr

    n, d = 8192 * 30 + 999, 8
    X = synth.generate(n, 0, n, d, 8, 99)
    b = _cdr.Context(ctx.device)
    try:
        ctx.load_points(X)
        ctx.seed_reset()
        ctx.seed_update(X[7])
        tot = _cdr.host_seq_sum(ctx.seed_block_sums())
        c_full = ctx.seed_scan(tot, 0.0)
        for cut in (8192 * 3, 8192 * 17):
            ctx.load_points(X[:cut])
            b.load_points(X[cut:])
            for s in (ctx, b):
                s.seed_reset()
                s.seed_update(X[7])
            bs0, bs1 = ctx.seed_block_sums(), b.seed_block_sums()
            assert _cdr.host_seq_sum(np.concatenate([bs0, bs1])) == tot
            c1 = ctx.seed_scan(tot, 0.0)
            ni, nf = b.seed_scan_begin(tot, float(np.sum(bs0)) / tot)
            assert ni > 0 and nf == 0
            prog = b.seed_scan_items(ni)
            c2, ok = _cdr.seed_program_eval(prog, c1)
            assert ok and c2 == c_full
            assert b.seed_scan_end(c1) == c_full
            u = 0.999
            i1, i2 = ctx.seed_search(c_full, u), b.seed_search(c_full, u)
            cdf = np.cumsum(np.sqrt(ko.sqdist_rows(X, X[7])) ** 2 / tot) / c_full
            want = int(np.searchsorted(cdf, u, side="right"))
            assert (i1 if i1 >= 0 else cut + i2) == want
    finally:
        b.close()


@pytest.mark.parametrize("n,d,k", [(150_000, 64, 24), (150_000, 32, 24), (200_000, 8, 16),
                                   (120_000, 16, 40)])
def test_seeding_fp16_certificate_vs_oracle(ctx, n, d, k):
    """The fp16-certified seeding update (csrc/seed_update.hip seed_update16c_kernel and seed_update16_kernel):
    minima it proves unchanged without the fp32 row must be exactly the ones
    the reference leaves unchanged — the seeds equal the reference run's,
    including with duplicated rows (zero distances, exact ties) and a far
    outlier (kmeans_plusplus.py:13-20)."""
    import kmeans_plusplus as kp

    X = synth.generate(n, 0, n, d, k, 31 * n + d)
    X[::97] = X[5]  # duplicates of one row
    X[n // 2] = X[n // 2] + 8.0  # an outlier
    init = kp.kmeans_plusplus_init(X, k, random_state=11, context=ctx)
    np.testing.assert_array_equal(init, ko.kmeans_plusplus_init(X, k, random_state=11))


def test_seeding_program_opaque_blocks(ctx):
    """Blocks the cumsum program cannot summarise (csrc/seed_scan.hip: more than
    32 binade crossings in a block -> FINE items walked element by element):
    a run of zero probabilities from a zero running value, and D^2 values
    growing 4x per row.  Seeds equal the reference's (kmeans_plusplus.py:
    13-20) on F64-mode data."""
    import kmeans_plusplus as kp

    n = 20000
    X = np.zeros((n, 2))
    X[8192 + 100: 8192 + 140, 0] = np.ldexp(1.0, np.arange(40) - 20)  # D^2 = 2^(2j - 40)
    X[15000:, 1] = np.linspace(0.0, 1.0, n - 15000)
    rs = next(r for r in range(100)
              if not 8192 + 100 <= int(np.random.default_rng(r).integers(0, n)) < 8192 + 140)
    for k in (2, 4, 6):
        init = kp.kmeans_plusplus_init(X, k, random_state=rs, context=ctx)
        np.testing.assert_array_equal(init, ko.kmeans_plusplus_init(X, k, random_state=rs))


def _drive_seed_shards(ctxs, begins, n_total, k, seed):
    """The device-resident sharded seeding (cdr_seed_shard_*) on several
    contexts of one GPU in lock step, the collectives done by device-tensor
    copies and sums between the phases (what RCCL does between ranks)."""
    import torch

    W, d = len(ctxs), ctxs[0].info()["d"]
    rng = np.random.default_rng(seed)
    first = int(rng.integers(0, n_total))
    u = rng.random(k - 1)
    red = [torch.zeros(d + 4, dtype=torch.float64, device="cuda") for _ in ctxs]

    def sync():
        for c in ctxs:
            c.synchronize()
        torch.cuda.synchronize()

    def allreduce():
        sync()
        tot = sum(red[1:], red[0].clone())
        for t in red:
            t.copy_(tot)
        torch.cuda.synchronize()

    def gather(bufs, m):
        sync()
        for r in range(W):
            for q in range(W):
                if q != r:
                    bufs[q][r * m:(r + 1) * m].copy_(bufs[r][r * m:(r + 1) * m])
        torch.cuda.synchronize()

    sizes = [c.seed_shard_begin(b, n_total, W, r, first, k, u, red[r].data_ptr())
             for r, (c, b) in enumerate(zip(ctxs, begins))]
    m0, m1 = int(sizes[0][0]), int(sizes[0][1])
    bs = [torch.zeros(W * m0, dtype=torch.uint8, device="cuda") for _ in ctxs]
    pg = [torch.zeros(W * m1, dtype=torch.uint8, device="cuda") for _ in ctxs]
    allreduce()
    for _ in range(1, k):
        for r, c in enumerate(ctxs):
            c.seed_shard_phase(0, red[r].data_ptr(), bs[r].data_ptr())
        gather(bs, m0)
        for r, c in enumerate(ctxs):
            c.seed_shard_phase(1, bs[r].data_ptr(), pg[r].data_ptr())
        gather(pg, m1)
        for r, c in enumerate(ctxs):
            c.seed_shard_phase(2, pg[r].data_ptr(), red[r].data_ptr())
        allreduce()
    return [c.seed_shard_end(red[r].data_ptr()) for r, c in enumerate(ctxs)]


@pytest.mark.parametrize("n,d,k,W", [(3 * 65536 + 1000, 16, 32, 2), (5 * 65536 + 77, 8, 24, 3),
                                     (2_000_000, 16, 64, 4)])
def test_sharded_device_seeding_contexts(ctx, n, d, k, W):
    """VERDICT r3 (missing 2): k-means++ over rows sharded on W contexts with
    every step on the devices (block sums all-gathered, cumsum programs
    all-gathered and composed on every rank, the picked row all-reduced):
    every rank's centres equal the single-shard device seeding and the
    oracle (kmeans_plusplus.py:3-22)."""
    import _cdr
    from cdr_dist import shard_rows

    X = synth.generate(n, 0, n, d, k, 1000 + n)
    ctx.load_points(X)
    rng = np.random.default_rng(42)
    first = int(rng.integers(0, n))
    want = ctx.get_rows(ctx.seed_run(first, k, rng.random(k - 1)))
    if n <= 400_000:
        np.testing.assert_array_equal(want, ko.kmeans_plusplus_init(X, k, random_state=42))
    ctxs = [_cdr.Context(ctx.device) for _ in range(W)]
    try:
        begins = []
        for r, c in enumerate(ctxs):
            b, m = shard_rows(n, W, r)
            c.load_points(X[b:b + m])
            begins.append(b)
        st = [c.points_stats() for c in ctxs]
        dd = (st[0].size - 3) // 2
        g = np.concatenate([np.minimum.reduce([s[:dd] for s in st]),
                            np.maximum.reduce([s[dd:] for s in st])])
        for c in ctxs:
            c.points_restat(g, n)
        outs = _drive_seed_shards(ctxs, begins, n, k, 42)
    finally:
        for c in ctxs:
            c.close()
    for picks, cents, status in outs:
        assert status == 0
        np.testing.assert_array_equal(cents, want)


class _ThreadComm:
    """The collectives of cdr_dist.Comm that the host seeding protocol uses
    (allgather, bcast, allreduce_i64, barrier), between threads of one
    process: each thread plays one rank with its own GPU context."""

    def __init__(self, hub, rank: int, world: int):
        self.hub, self.rank, self.world = hub, rank, world
        self.dist, self.device, self.seed_bad = True, None, 0

    def _exchange(self, val):
        self.hub["slots"][self.rank] = val
        self.hub["bar"].wait()
        out = list(self.hub["slots"])
        self.hub["bar"].wait()
        return out

    def allgather(self, arr):
        return [np.array(x, copy=True) for x in self._exchange(np.asarray(arr))]

    def bcast(self, arr, src: int):
        return np.array(self._exchange(np.asarray(arr))[src], copy=True)

    def allreduce_i64(self, arr, op: str = "sum"):
        parts = np.stack(self._exchange(np.asarray(arr, dtype=np.int64)))
        return {"sum": parts.sum(0), "min": parts.min(0), "max": parts.max(0)}[op]

    def barrier(self):
        self.hub["bar"].wait()


def test_sharded_device_seeding_status1_falls_back(ctx):
    """ADVICE r4 #3 / VERDICT r5: a shard whose cumsum program cannot be
    composed (an opaque block: D^2 growing 4x per row, more binade crossings
    than a program item list holds) makes the device-resident sharded seeding
    report status 1 on EVERY context; the host protocol the ranks then run
    together (cdr_dist.seed_host_protocol, here one thread per rank) gives the
    reference's centres (kmeans_plusplus.py:13-20)."""
    import threading

    import _cdr
    from cdr_dist import seed_host_protocol, shard_rows

    n, k, seed, W = 20000, 4, 3, 2
    X = np.zeros((n, 2))
    base = 2 * 8192 + 100  # in the last shard's block: its start is a guess
    X[base:base + 40, 0] = np.ldexp(1.0, np.arange(40) - 20)  # D^2 = 2^(2j - 40)
    X[12000:, 1] = np.linspace(0.0, 1.0, n - 12000)
    want = ko.kmeans_plusplus_init(X, k, random_state=seed)
    ctxs = [_cdr.Context(ctx.device) for _ in range(W)]
    try:
        begins = []
        for r, c in enumerate(ctxs):
            b, m = shard_rows(n, W, r)
            c.load_points(X[b:b + m])
            begins.append(b)
        st = [c.points_stats() for c in ctxs]
        dd = (st[0].size - 3) // 2
        g = np.concatenate([np.minimum.reduce([s[:dd] for s in st]),
                            np.maximum.reduce([s[dd:] for s in st])])
        for c in ctxs:
            c.points_restat(g, n)
        outs = _drive_seed_shards(ctxs, begins, n, k, seed)
        assert [o[2] for o in outs] == [1] * W, [o[2] for o in outs]
        rng = np.random.default_rng(seed)
        first = int(rng.integers(0, n))
        u = rng.random(k - 1)
        hub = {"slots": [None] * W, "bar": threading.Barrier(W)}
        res, errs = [None] * W, []

        def rank_main(r):
            try:
                res[r] = seed_host_protocol(ctxs[r], _ThreadComm(hub, r, W),
                                            np.array(begins, dtype=np.int64), n, first, k, u,
                                            _cdr.host_seq_sum)
            except BaseException as e:  # noqa: BLE001 - reported below
                errs.append(e)
                hub["bar"].abort()

        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(W)]
        for t in th:
            t.start()
        for t in th:
            t.join(120)
        assert not errs, errs
    finally:
        for c in ctxs:
            c.close()
    for r in range(W):
        np.testing.assert_array_equal(res[r], want)


def test_sharded_device_seeding_native_world1(ctx):
    """cdr_seed_run_sharded: the same phases with the collectives issued from
    C (ncclAllGather / ncclAllReduce on a one-rank communicator) equal the
    single-shard device seeding."""
    import _cdr

    n, d, k = 600_000, 16, 48
    X = synth.generate(n, 0, n, d, k, 4321)
    ctx.load_points(X)
    rng = np.random.default_rng(7)
    first = int(rng.integers(0, n))
    u = rng.random(k - 1)
    want = ctx.get_rows(ctx.seed_run(first, k, u))
    b = _cdr.Context(ctx.device)
    try:
        b.load_points(X)
        b.comm_init(_cdr.comm_unique_id(), 1, 0)
        assert b.comm_ranks() == (1, 0)
        picks, cents, status = b.seed_run_sharded(0, n, first, k, u)
        assert status == 0
        np.testing.assert_array_equal(cents, want)
        b.comm_destroy()
        assert b.comm_ranks()[0] == 0
    finally:
        b.close()

"""The contingency table of two labelings on the device (csrc/agree.hip,
cluster_agreement.py) equals contingency_host's integers, in both kernel
forms; the kept labels, the errors, cluster_quality.stability and the CLI's
--previous_plan."""
import glob
import json
import os

import numpy as np
import pandas as pd
import pytest

import plan_cases as pc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")
GOLDEN_CSV = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
LDS, GLOBAL = 0, 1
LDS_ROWS = 1024 * 4     # rows of one agree_lds workgroup iteration (16 waves x 4 groups of 64)
GLOBAL_ROWS = 256 * 4   # rows of one agree_global workgroup iteration
SIZE_EDGES = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62], dtype=np.int64)
FORMS_SEEN = set()


def mixed_sizes(rng, n):
    return np.where(rng.random(n) < 0.5, SIZE_EDGES[rng.integers(0, len(SIZE_EDGES), n)],
                    rng.integers(0, 2 ** 63, n, dtype=np.int64)).astype(np.int64)


def check(ctx, a, b, ka, kb, sizes=None, form=None):
    """The device's table of (a, b) is the definition's; the form is `form`."""
    from cluster_agreement import contingency, contingency_host

    want = contingency_host(a, b, ka, kb, sizes)
    got = contingency(a, b, ka=ka, kb=kb, sizes=sizes, context=ctx)
    info = ctx.agree_info()
    if sizes is None:
        assert got.dtype == np.int64 and got.shape == (ka, kb)
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1].shape == (ka, kb) and (got[1] == want[1]).all()
        assert sum(got[1].ravel().tolist()) == sum(int(s) for s in np.asarray(sizes).tolist())
    cap = info["cap_sizes"] if sizes is not None else info["cap_counts"]
    expect = LDS if ka * kb <= cap else GLOBAL
    assert info["form"] == expect and (form is None or form == expect), (info, ka, kb)
    if len(a):
        FORMS_SEEN.add(expect)
    return info


def shape_of(cells):
    """(ka, kb) with ka * kb == cells and both at most 1024, or None."""
    for ka in range(max(1, -(-cells // 1024)), 1025):
        if cells % ka == 0 and cells // ka <= 1024:
            return ka, cells // ka
    return None


def shape_from(cells, step):
    while shape_of(cells) is None:
        cells += step
    return shape_of(cells)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                               262144, 262145, 300000])
def test_row_counts(ctx, n):
    """A partial wave, a partial group of four 64-row groups, a partial
    workgroup iteration (1024 rows in the global form, 4096 in the LDS form) and
    several workgroups, in both forms with and without sizes."""
    rng = np.random.default_rng(n)
    sizes = mixed_sizes(rng, n)
    for ka, kb, s, form in ((5, 7, None, LDS), (5, 7, sizes, LDS), (130, 127, None, GLOBAL),
                            (65, 64, sizes, GLOBAL)):
        info = check(ctx, rng.integers(0, ka, n), rng.integers(0, kb, n), ka, kb, s, form)
        rows = LDS_ROWS if form == LDS else GLOBAL_ROWS
        assert info["workgroups"] <= -(-n // rows)
        assert info["workgroups"] == -(-n // rows) or info["workgroups"] >= 256


def test_the_first_row_past_the_full_grid(ctx):
    """The grid stops growing at a multiple of the CU count (at most 1024
    workgroups in the LDS form): with G workgroups of R rows per iteration, row
    G * R is the first one a workgroup reaches in its second iteration.  G is
    read from agree_info after a call large enough to fill the grid.  (R is
    4096 in the LDS form and 1024 in the global form, not plan_size_sums' 256,
    so 262144 and 262145 in test_row_counts are not that edge here.)"""
    rng = np.random.default_rng(5)
    big = 1 << 22
    for ka, kb, form, rows in ((6, 5, LDS, LDS_ROWS), (130, 127, GLOBAL, GLOBAL_ROWS)):
        a, b = rng.integers(0, ka, big), rng.integers(0, kb, big)
        assert ctx.agree_table(ka, kb, a, b).sum() == big
        grid = ctx.agree_info()["workgroups"]
        assert grid * rows < big and (form != LDS or grid <= 1024)
        for n in (grid * rows, grid * rows + 1):
            assert check(ctx, a[:n], b[:n], ka, kb, None, form)["workgroups"] == grid
        n = grid * rows + 1
        check(ctx, a[:n], b[:n], ka, kb, mixed_sizes(rng, n), form)


@pytest.mark.parametrize("ka,kb", [(1, 1), (1, 1024), (1024, 1), (2, 3), (64, 64), (65, 64),
                                   (1024, 1024)])
@pytest.mark.parametrize("with_sizes", [False, True])
def test_shapes(ctx, ka, kb, with_sizes):
    n = 5000
    rng = np.random.default_rng(ka * 1031 + kb)
    a, b = rng.integers(0, ka, n), rng.integers(0, kb, n)
    a[0], b[0], a[-1], b[-1] = ka - 1, kb - 1, 0, 0  # the table's last and first cell
    check(ctx, a, b, ka, kb, mixed_sizes(rng, n) if with_sizes else None)


@pytest.mark.parametrize("with_sizes", [False, True])
def test_both_sides_of_the_lds_cap(ctx, with_sizes):
    """Tables of exactly the LDS cap's cells and of the first cell count past it
    that two factors of at most 1024 give, every cell hit."""
    info = ctx.agree_info()
    cap = info["cap_sizes"] if with_sizes else info["cap_counts"]
    assert info["cap_sizes"] >= 4096 and info["cap_counts"] >= info["cap_sizes"]
    rng = np.random.default_rng(cap)
    for (ka, kb), form in ((shape_from(cap, -1), LDS), (shape_from(cap + 1, 1), GLOBAL)):
        n = 3 * ka * kb
        cell = rng.permutation(n) % (ka * kb)
        check(ctx, cell // kb, cell % kb, ka, kb, mixed_sizes(rng, n) if with_sizes else None, form)
    assert FORMS_SEEN == {LDS, GLOBAL}


@pytest.mark.parametrize("ka,kb,with_sizes,form", [(64, 64, False, LDS), (64, 64, True, LDS),
                                                   (1024, 1024, False, GLOBAL),
                                                   (65, 64, True, GLOBAL)])
def test_contention(ctx, ka, kb, with_sizes, form):
    """All rows in one cell, rows sorted by cell (whole 64-row groups in one
    cell, and groups that straddle two), two labelings equal up to a
    permutation, independent uniform labelings."""
    n = 70001
    rng = np.random.default_rng(ka + kb)
    sizes = mixed_sizes(rng, n) if with_sizes else None
    one_a, one_b = np.full(n, ka - 1), np.full(n, kb - 2)
    check(ctx, one_a, one_b, ka, kb, sizes, form)
    k = min(ka, kb)
    a = np.sort(rng.integers(0, k, n))
    perm = rng.permutation(kb)
    check(ctx, a, a, ka, kb, sizes, form)
    check(ctx, a, perm[a], ka, kb, sizes, form)
    shuffled = rng.permutation(a)
    check(ctx, shuffled, perm[shuffled], ka, kb, sizes, form)
    check(ctx, rng.integers(0, ka, n), rng.integers(0, kb, n), ka, kb, sizes, form)
    holes = a.copy()  # groups that mix a sorted run with rows of another cluster
    holes[::3] = ka - 1
    check(ctx, holes, perm[a], ka, kb, sizes, form)


def test_sizes_past_uint64(ctx):
    """300000 rows of 2^62 bytes in one cell: 300000 * 2^62 > 2^64, what the
    low / high split is for; and every edge size alone."""
    from cluster_agreement import contingency

    n = 300000
    a, b = np.zeros(n, dtype=np.int64), np.full(n, 2)
    for ka, kb in ((2, 3), (70, 60)):
        counts, nbytes = contingency(a, b, ka=ka, kb=kb, sizes=np.full(n, 2 ** 62), context=ctx)
        assert counts[0, 2] == n and counts.sum() == n
        assert nbytes[0, 2] == n * 2 ** 62 and nbytes[0, 2] > 2 ** 64
        assert sum(nbytes.ravel().tolist()) == n * 2 ** 62
    for s in SIZE_EDGES.tolist() + [2 ** 63 - 1]:
        check(ctx, [1, 0, 1], [0, 2, 0], 2, 3, [s, 5, s], LDS)
        check(ctx, [1, 0, 1], [0, 2, 0], 70, 60, [s, 5, s], GLOBAL)


def blobs(n, d, k, seed, spread=0.05):
    rng = np.random.default_rng(seed)
    centres = rng.random((k, d)) * 100.0
    return centres[rng.integers(0, k, n)] + rng.normal(0.0, spread, (n, d))


def test_resident_and_kept_labels(ctx):
    import kmeans_plusplus as kp
    from cluster_agreement import contingency, contingency_host, keep

    X = np.random.default_rng(3).random((700, 5))
    np.random.seed(0)
    _, first = kp.kmeans(X, 4, random_state=1, context=ctx)
    keep(context=ctx)
    _, second = kp.kmeans(X, 5, random_state=2, context=ctx)
    assert ctx.labels().tolist() == second.tolist()
    want = contingency_host(second, first, 5, 4)
    assert want.sum() == 700 and np.count_nonzero(want) > 5
    np.testing.assert_array_equal(contingency(ka=5, kb=4, context=ctx), want)
    np.testing.assert_array_equal(contingency(second, first, ka=5, kb=4, context=ctx), want)
    np.testing.assert_array_equal(contingency(None, first, ka=5, kb=4, context=ctx), want)
    np.testing.assert_array_equal(contingency(second, None, ka=5, kb=4, context=ctx), want)
    sizes = mixed_sizes(np.random.default_rng(4), 700)
    got = contingency(ka=8, kb=1024, sizes=sizes, context=ctx)  # a wider table, the global form
    ref = contingency_host(second, first, 8, 1024, sizes)
    np.testing.assert_array_equal(got[0], ref[0])
    assert (got[1] == ref[1]).all() and ctx.agree_info()["form"] == GLOBAL
    with pytest.raises(ValueError, match="smaller than the resident"):
        contingency(ka=4, kb=4, context=ctx)
    with pytest.raises(ValueError, match="smaller than the kept"):
        contingency(ka=5, kb=3, context=ctx)
    # the kept labels survive other points and other labels
    ctx.load_points(np.random.default_rng(5).random((60, 5)))
    np.testing.assert_array_equal(contingency(second, None, ka=5, kb=4, context=ctx), want)
    with pytest.raises(RuntimeError, match="no labels"):
        contingency(ka=5, kb=4, context=ctx)
    _, other = kp.kmeans(np.random.default_rng(5).random((60, 5)), 3, random_state=1, context=ctx)
    with pytest.raises(ValueError, match="row count"):
        contingency(ka=5, kb=4, context=ctx)  # 60 resident rows against 700 kept
    with pytest.raises(ValueError, match="row count"):
        contingency(other, None, ka=5, kb=4, context=ctx)
    np.testing.assert_array_equal(contingency(second, None, ka=5, kb=4, context=ctx), want)
    keep(context=ctx)  # another keep replaces them
    np.testing.assert_array_equal(contingency(ka=3, kb=3, context=ctx),
                                  contingency_host(other, other, 3, 3))


def test_errors_leave_the_context_usable(ctx):
    import _cdr
    from cluster_agreement import contingency

    n = 3000
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 6, n), rng.integers(0, 7, n)
    sizes = rng.integers(0, 2 ** 40, n).astype(np.int64)

    def ok():
        check(ctx, a, b, 6, 7, sizes, LDS)
        check(ctx, a, b, 160, 110, None, GLOBAL)

    for ka, kb in ((6, 7), (160, 110)):  # both forms flag on the device
        for side in (0, 1):
            for value in (-1, (ka, kb)[side], 2 ** 40, -2 ** 40):
                bad = [a.copy(), b.copy()]
                bad[side][1234] = value
                with pytest.raises(ValueError, match="label"):
                    contingency(bad[0], bad[1], ka=ka, kb=kb, context=ctx)
                with pytest.raises(ValueError, match="label"):
                    contingency(bad[0], bad[1], ka=ka, kb=kb, sizes=sizes, context=ctx)
            ok()
        neg = sizes.copy()
        neg[n - 1] = -1
        with pytest.raises(ValueError, match="negative size"):
            contingency(a, b, ka=ka, kb=kb, sizes=neg, context=ctx)
        ok()
    for ka, kb in ((0, 7), (6, 0), (1025, 7), (6, 1025), (-1, 7)):
        with pytest.raises(NotImplementedError):
            contingency(a, b, ka=ka, kb=kb, context=ctx)
    ok()
    with pytest.raises(ValueError, match="differ in length"):
        contingency(a, b[:-1], ka=6, kb=7, context=ctx)
    with pytest.raises(ValueError, match="differ in length"):
        contingency(a, b, ka=6, kb=7, sizes=sizes[:-1], context=ctx)
    lib, h = ctx._lib, ctx._h
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    counts = np.zeros((6, 7), dtype=np.uint64)
    sums = np.zeros((6, 7, 2), dtype=np.uint64)
    p = _cdr._ptr
    assert lib.cdr_agree_table(h, p(a64), 6, p(b64), 7, n, None, p(counts), p(sums)) == _cdr.CDR_ERR_ARG
    assert b"size_sums without sizes" in lib.cdr_last_error()
    assert lib.cdr_agree_table(h, p(a64), 6, p(b64), 7, -1, None, p(counts), None) == _cdr.CDR_ERR_ARG
    assert lib.cdr_agree_table(h, p(a64), 6, p(b64), 7, 2 ** 31, None, p(counts), None) == _cdr.CDR_ERR_ARG
    counts[...] = 7
    assert lib.cdr_agree_table(h, p(a64), 6, p(b64), 7, 0, None, p(counts), None) == _cdr.CDR_OK
    assert not counts.any()  # n = 0: a zero table
    ok()
    fresh = _cdr.Context(ctx.device)
    try:
        with pytest.raises(RuntimeError, match="no labels"):
            fresh.agree_keep()
        with pytest.raises(RuntimeError, match="no kept labels"):
            fresh.agree_table(6, 7, a, None)
        with pytest.raises(RuntimeError, match="no labels"):
            fresh.agree_table(6, 7, None, b)
        assert fresh.agree_info()["form"] == -1
        np.testing.assert_array_equal(fresh.agree_table(6, 7, a, b), ctx.agree_table(6, 7, a, b))
        assert fresh.agree_table(6, 7, [], []).tolist() == [[0] * 7] * 6
    finally:
        fresh.close()
    t = ctx.agree_timing()
    assert t.shape == (3,) and (t >= 0).all() and t[1] > 0


def test_resident_state_untouched(ctx, tmp_path):
    from cluster_agreement import contingency, keep
    from features_csv import kmeans_csv

    np.random.seed(0)
    C, labels = kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)
    step = ctx.lloyd_step_f64 if ctx.info()["mode"] == 2 else ctx.lloyd_step

    def state():
        return ctx.labels(), ctx.medians_by_label(4), step(C), ctx.get_rows(np.arange(50))

    data = pc.read(GOLDEN_CSV)
    body = data.index(b"\n") + 1
    tails = pc.tails_of("abcd", [1, 2, 3, 4])
    whole = ctx.plan_format(data, body, 11, 0, None, 4, tails)["text"].tobytes()
    before = state()
    head = ctx.plan_format(data, body, 11, 0, None, 4, tails, 0, 10)["text"].tobytes()
    keep(context=ctx)
    rng = np.random.default_rng(1)
    table = contingency(ka=4, kb=4, sizes=np.arange(50), context=ctx)
    assert np.array_equal(table[0], np.diag(np.bincount(before[0], minlength=4)))
    contingency(rng.integers(0, 200, 5000), rng.integers(0, 200, 5000), ka=200, kb=200, context=ctx)
    with pytest.raises(ValueError):
        contingency(np.full(50, 4), None, ka=4, kb=4, context=ctx)
    # the plan's record index and its labels are still on the device: the next chunk
    rest = ctx.plan_format(data, body, 11, 0, None, 4, tails, 10, 1000)["text"].tobytes()
    assert head + rest == whole
    after = state()
    for x, y in zip(before, after):
        for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


def test_stability(ctx):
    import kmeans_plusplus as kp
    from cluster_agreement import adjusted_rand, contingency_host
    from cluster_quality import stability

    seeds = [1, 2, 3, 4]
    X = blobs(900, 5, 3, seed=2)
    res = stability(X, 3, seeds, context=ctx)
    assert res == {"k": 3, "ari": [1.0, 1.0, 1.0], "mean": 1.0, "min": 1.0}
    X = np.random.default_rng(8).random((900, 5))  # no structure: the seeds disagree
    np.random.seed(0)
    res = stability(X, 6, seeds, context=ctx)
    np.random.seed(0)
    labels = [kp.kmeans(X, 6, random_state=s, context=ctx)[1] for s in seeds]
    want = [adjusted_rand(contingency_host(l, labels[0], 6, 6)) for l in labels[1:]]
    assert res["ari"] == want and min(want) < 1.0
    assert res["mean"] == float(np.mean(want)) and res["min"] == min(want) and res["k"] == 6
    with pytest.raises(NotImplementedError):
        stability(X, 6, seeds, context=ctx, comm=object())
    with pytest.raises(ValueError):
        stability(X, 6, [1], context=ctx)


def run_cli(ctx, capsys, tmp_path, *extra):
    import replication_plan

    out = str(tmp_path / f"plan{len(os.listdir(tmp_path))}.csv")
    np.random.seed(0)
    replication_plan.main(["--input_path", os.path.join(PDIR, "features_out"), "--k", "4",
                           "--tables", os.path.join(PDIR, "main_tables.json"), "--out", out,
                           *extra], context=ctx)
    return out, capsys.readouterr().out


def test_cli_previous_plan(ctx, tmp_path, capsys):
    manifest = os.path.join(PDIR, "metadata.csv")
    first, base_text = run_cli(ctx, capsys, tmp_path, "--manifest", manifest, "--current_factor", "3")
    _, bare_text = run_cli(ctx, capsys, tmp_path)
    plan = pd.read_csv(first)
    size_of = pd.read_csv(manifest).drop_duplicates("path").set_index("path")["size_bytes"]
    total = int(sum(int(size_of[p]) for p in plan["path"]))
    # the same plan both days: nothing moves
    second, text = run_cli(ctx, capsys, tmp_path, "--manifest", manifest, "--current_factor", "3",
                           "--previous_plan", first)
    assert pc.read(second) == pc.read(first)
    assert text.replace(os.path.basename(second), "X").startswith(
        base_text.replace(os.path.basename(first), "X"))  # the lines before it are unchanged
    lines = text.strip().split("\n")
    assert len(lines) == len(base_text.strip().split("\n")) + 1
    same = json.loads(lines[-1])
    assert same["total"] == {"files": 50, "bytes": total, "bytes_to_copy": 0, "bytes_to_free": 0,
                             "files_changed": 0}
    assert all(list(v) == [c] for c, v in same["moves"].items())
    # without a manifest: one JSON line, files only
    _, text = run_cli(ctx, capsys, tmp_path, "--previous_plan", first)
    assert len(text.strip().split("\n")) == len(bare_text.strip().split("\n")) + 1
    assert json.loads(text.strip().split("\n")[-1])["total"] == {"files": 50, "files_changed": 0}
    # yesterday's plan with the clusters' categories rotated and ten files missing
    cat_of = plan.drop_duplicates("cluster").set_index("cluster")[["category", "replication"]]
    clusters = sorted(cat_of.index)
    turn = {c: clusters[(i + 1) % len(clusters)] for i, c in enumerate(clusters)}
    prev = plan.copy()
    prev["category"] = [cat_of["category"][turn[c]] for c in plan["cluster"]]
    prev["replication"] = [int(cat_of["replication"][turn[c]]) for c in plan["cluster"]]
    prev = prev.iloc[10:]
    prev_path = str(tmp_path / "prev.csv")
    prev.to_csv(prev_path, index=False)
    want, tot = {}, dict(files=0, bytes=0, bytes_to_copy=0, bytes_to_free=0, files_changed=0)
    old = prev.set_index("path")
    for p, c, f in zip(plan["path"], plan["category"], plan["replication"]):
        oc, of = (old["category"][p], int(old["replication"][p])) if p in old.index else ("(new)", 2)
        s, f = int(size_of[p]), int(f)
        row = want.setdefault(oc, {}).setdefault(c, dict(old_factor=of, new_factor=f, files=0, bytes=0,
                                                         bytes_to_copy=0, bytes_to_free=0))
        add = dict(files=1, bytes=s, bytes_to_copy=max(f - of, 0) * s, bytes_to_free=max(of - f, 0) * s)
        for key, v in add.items():
            row[key] += v
            tot[key] += v
        tot["files_changed"] += of != f
    _, text = run_cli(ctx, capsys, tmp_path, "--manifest", manifest, "--current_factor", "2",
                      "--previous_plan", prev_path)
    assert json.loads(text.strip().split("\n")[-1]) == {"moves": want, "total": tot}
    assert "(new)" in want and tot["files"] == 50
    with pytest.raises(SystemExit, match="10 paths are not in the previous plan"):
        run_cli(ctx, capsys, tmp_path, "--previous_plan", prev_path)
    broken = plan.copy()
    broken.loc[broken.index[-1], "replication"] = 99
    broken.to_csv(prev_path, index=False)
    with pytest.raises(SystemExit, match="more than one category or factor"):
        run_cli(ctx, capsys, tmp_path, "--previous_plan", prev_path)

"""The replication plan written on the device (csrc/plan.hip, replication_plan.py)
equals write_plan_csv_host's bytes, and cdr_plan_size_sums equals Python ints."""
import glob
import json
import os
import random

import numpy as np
import pandas as pd
import pytest

import csv_read_cases as rc
import plan_cases as pc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")
GOLDEN_CSV = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
TILE = 4096         # bytes per tile of the record index (csvin.hip kTile)
SCAN_PART = 4096    # tiles per workgroup of the index scan (kScanPart)


def both(ctx, tmp_path, data, labels, cats=pc.CATS4, factors=pc.FACTORS, resident=False, **kw):
    """(device file, host file, info) of one input."""
    from replication_plan import write_plan_csv, write_plan_csv_host

    src = pc.put(tmp_path / "f.csv", data)
    info = {}
    write_plan_csv(src, str(tmp_path / "dev.csv"), cats, factors,
                   labels=None if resident else labels, context=ctx, info=info, **kw)
    write_plan_csv_host(src, str(tmp_path / "host.csv"), cats, factors, labels=labels,
                        **{k: v for k, v in kw.items() if k != "chunk_rows"})
    return pc.read(tmp_path / "dev.csv"), pc.read(tmp_path / "host.csv"), info


def same(dev, host):
    if dev != host:
        at = next((i for i, (a, b) in enumerate(zip(dev, host)) if a != b), min(len(dev), len(host)))
        raise AssertionError((len(dev), len(host), at, dev[max(at - 60, 0):at + 60], host[max(at - 60, 0):at + 60]))


def clean(info, rows):
    """No deferred row and no fallback: the kernels wrote every byte."""
    assert info["rows"] == rows and info["deferred_rows"] == 0, info
    assert info["whole_file_fallback"] is False, info


def golden_tables():
    with open(os.path.join(PDIR, "main_tables.json")) as fh:
        t = json.load(fh)
    final = pd.read_csv(os.path.join(PDIR, "final_categories.csv"))
    return t, {f"C{j}": c for j, c in enumerate(final["category"])}


def test_golden_pipeline_file_resident_and_explicit_labels(ctx, tmp_path):
    from features_csv import kmeans_csv
    from replication_plan import write_plan_csv, write_plan_csv_host

    t, cats = golden_tables()
    np.random.seed(0)
    _, labels = kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)
    np.testing.assert_array_equal(labels, np.load(os.path.join(PDIR, "main_kmeans.npz"))["labels"])
    host = str(tmp_path / "host.csv")
    assert write_plan_csv_host(GOLDEN_CSV, host, cats, t["REPLICATION_FACTORS"], labels=labels) == 50
    for lab in (None, labels):
        info = {}
        out = str(tmp_path / "dev.csv")
        assert write_plan_csv(GOLDEN_CSV, out, cats, t["REPLICATION_FACTORS"], labels=lab,
                              context=ctx, info=info) == 50
        same(pc.read(out), pc.read(host))
        clean(info, 50)
        assert all(k in info for k in ("upload_ms", "index_ms", "length_ms", "emit_ms", "copy_ms"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537])
def test_row_counts(ctx, tmp_path, n):
    """The workgroup (256 rows), the wave (64 rows) and the one-workgroup scan
    (256 workgroup sums: 65 536 rows) edges."""
    data = pc.plain_file(n, seed=n, path=lambda i: f"/d/{i % 89}/f{i}")
    dev, host, info = both(ctx, tmp_path, data, pc.labels_for(n, 4, seed=n))
    same(dev, host)
    clean(info, n)


def test_labels_of_one_to_four_digits_factors_and_categories(ctx, tmp_path):
    """k = 1024 with every label present, label 0 and k - 1 at the first and
    last row; factors of 1 and 3 digits and 0; categories of 1 and 40 bytes."""
    k, n = 1024, 3000
    names = ["H", "M" * 40, "Zero", "Big"]
    factors = {"H": 3, "M" * 40: 1, "Zero": 0, "Big": 125}
    cats = {f"C{j}": names[j % 4] for j in range(k)}
    for first, last in ((0, k - 1), (k - 1, 0)):
        labels = np.arange(n, dtype=np.int64) % k
        np.random.default_rng(5).shuffle(labels)
        labels[0], labels[-1] = first, last
        assert len(set(labels.tolist())) == k
        dev, host, info = both(ctx, tmp_path, pc.plain_file(n, seed=9), labels, cats, factors)
        same(dev, host)
        clean(info, n)
    dev, host, info = both(ctx, tmp_path, pc.plain_file(10), np.zeros(10, dtype=np.int64),
                           {"C0": "H"}, factors)  # k = 1
    same(dev, host)
    clean(info, 10)


@pytest.mark.parametrize("col", [0, 5, 10])
def test_paths_of_every_kind_and_the_path_column_anywhere(ctx, tmp_path, col):
    n = 400
    rows = rc.table_text(n, rc.HEADER11, seed=21)
    special = {0: "", 1: "x", 2: "/données/ß€/файл.bin", 3: "/with space/and\ttab ", 4: " lead",
               5: "/long/" + "p" * 5000, 6: "NA", 7: "nan", 8: "1.50", 200: "", 255: "y" * pc.MAX_FIELD,
               256: "/semi;colon'", n - 1: ""}
    for r, p in special.items():
        rows[r][0] = p
    names = list(rc.HEADER11)
    if col:  # the path column moves; the rows keep 11 fields
        names.insert(col, names.pop(0))
        rows = [r[1:col + 1] + [r[0]] + r[col + 1:] for r in rows]
    lines = [",".join(names)] + [",".join(r) for r in rows]
    data = ("\n".join(lines) + "\n").encode("utf-8")
    dev, host, info = both(ctx, tmp_path, data, pc.labels_for(n, 4, seed=3))
    same(dev, host)
    clean(info, n)


def test_a_path_past_the_field_limit_is_deferred(ctx, tmp_path):
    rows = rc.table_text(300, rc.HEADER11, seed=23)
    rows[100][0] = "z" * (pc.MAX_FIELD + 1)
    rows[101][0] = "z" * pc.MAX_FIELD
    dev, host, info = both(ctx, tmp_path, rc.file_bytes(rc.HEADER11, rows), pc.labels_for(300, 4))
    same(dev, host)
    assert info["deferred_rows"] == 1 and info["whole_file_fallback"] is False


@pytest.mark.parametrize("eol,last_eol,blanks", [(b"\r\n", True, False), (b"\n", False, False),
                                                 (b"\r\n", False, False), (b"\n", True, True),
                                                 (b"\r\n", True, True)])
def test_line_ends_and_blank_lines(ctx, tmp_path, eol, last_eol, blanks):
    rows = rc.table_text(200, rc.HEADER11, seed=7)
    data = rc.file_bytes(rc.HEADER11, rows, eol=eol, last_eol=last_eol)
    if blanks:
        lines = data.split(eol)
        lines[1:1] = [b""]
        lines[50:50] = [b"", b""]
        data = eol.join(lines) + eol + eol
    dev, host, info = both(ctx, tmp_path, data, pc.labels_for(200, 4))
    same(dev, host)
    clean(info, 200)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("shift", [0, 1, 2, 7])
def test_rows_at_the_tile_edge(ctx, tmp_path, eol, shift):
    rows = rc.table_text(120, rc.HEADER11, seed=11)
    lens = np.cumsum([len(",".join(r).encode()) + len(eol) for r in rows])
    j = int(np.searchsorted(lens, TILE)) + 1
    target = TILE + shift + (1 if eol == b"\r\n" and shift == 0 else 0)
    rows[j][0] += "x" * (target + TILE - int(lens[j]))
    data = rc.file_bytes(rc.HEADER11, rows, eol=eol)
    body = data[len(",".join(rc.HEADER11).encode() + eol):]
    end = len(eol.join(",".join(r).encode() for r in rows[:j + 1])) + len(eol)
    assert end == 2 * TILE + target - TILE and body[end - 1:end] == b"\n"
    dev, host, info = both(ctx, tmp_path, data, pc.labels_for(120, 4))
    same(dev, host)
    clean(info, 120)


def test_more_than_one_scan_part(ctx, tmp_path):
    """Just over 16 MiB of short rows (test_gpu_csv_read's file shape): the
    index scan runs over several parts and quotes far apart carry their parity."""
    rng = random.Random(17)
    block = [f"p{i},{rc.numeric_text(rng, 0.5)}\n".encode() for i in range(5000)]
    text = b"".join(block)
    reps = (SCAN_PART * TILE + 200000) // len(text) + 1
    quoted = [b'"a,b",0.25\n', b'"two\nlines",0.5\n', b'"q""q",0.75\n']
    parts, marks = [b"k,v\n"], []
    for r in range(reps):
        if r in (1, reps // 2, reps - 1):
            marks.append(r * len(block) + len(marks))
            parts.append(quoted[len(marks) - 1])
        parts.append(text)
    data = b"".join(parts)
    n = reps * len(block) + 3
    dev, host, info = both(ctx, tmp_path, data, pc.labels_for(n, 4, seed=1), path_column="k")
    same(dev, host)
    assert info["rows"] == n and info["deferred_rows"] == 3 and info["whole_file_fallback"] is False


def test_deferred_rows_are_exactly_the_injected_ones(ctx, tmp_path):
    n = 600
    rows = rc.table_text(n, rc.HEADER11, seed=23)
    special = {0: "/a,b", 255: '/q""uote', 256: "/two\nlines", 257: 'x,"y"\n,z', 300: "/nul\0x",
               n - 1: "/last,one"}
    for r, p in special.items():
        rows[r][0] = p
    rows[511] = rows[511][:9]            # ragged: short
    rows[512] = rows[512] + ["1", "2"]   # ragged: long
    data = rc.file_bytes(rc.HEADER11, rows).replace(b'/q""""uote', b'/q""uote')
    marked = sorted(list(special) + [511, 512])
    labels = pc.labels_for(n, 4, seed=4)
    body = data.index(b"\n") + 1
    res = ctx.plan_format(data, body, 11, 0, labels, 4, pc.tails_of(["a", "b", "c", "d"], [1, 2, 3, 4]))
    assert res["rows"] == n and res["guard"] == -1
    assert res["deferred"][:, 0].tolist() == marked and res["deferred_rows"] == len(marked)
    records, _ = rc.split_records(data[body:])
    for r, off, b0, b1 in res["deferred"]:
        assert data[b0:b1].lstrip(b"\n") == data[body + records[r][0]:body + records[r][1]]
    # (pandas ends the NUL row's path at the NUL: the splice takes the definition's text)
    dev, host, info = both(ctx, tmp_path, data, labels)
    same(dev, host)
    assert info["deferred_rows"] == len(marked) and info["whole_file_fallback"] is False


GUARDS = [b'/a"b', b'"a"x', b' "q"']


@pytest.mark.parametrize("case", range(5))
def test_guard_cases_take_the_whole_file(ctx, tmp_path, case):
    """The cases of test_gpu_csv_read's test_guard_offsets_and_the_whole_file_path.
    Cases 0 and 4 leave the file inside quotes, so the device sees data rows
    0..99 and one tail record; case 3's line of blanks is a record for it."""
    from replication_plan import write_plan_csv, write_plan_csv_host

    rows = rc.table_text(150, rc.HEADER11, seed=31)
    lines = rc.file_bytes(rc.HEADER11, rows).split(b"\n")
    at = sum(len(ln) + 1 for ln in lines[:101])  # file offset of data row 100
    if case < 3:
        lines[101] = GUARDS[case] + lines[101][lines[101].index(b","):]
        off = [2, 2, 1][case]
    elif case == 3:
        lines[101:101] = [b" \t "]
        off = 0
    else:
        lines[101] = b'"open' + lines[101][lines[101].index(b","):]
        off = 0
    data = b"\n".join(lines)
    labels = pc.labels_for(150, 4)
    device_rows = {0: 101, 1: 150, 2: 150, 3: 151, 4: 101}[case]
    res = ctx.plan_format(data, data.index(b"\n") + 1, 11, 0, np.resize(labels, device_rows), 4,
                          pc.tails_of("abcd", [1, 2, 3, 4]))
    assert res["rows"] == device_rows and res["guard"] == at + off, (res["rows"], res["guard"], at, off)
    if case == 4:
        src = pc.put(tmp_path / "g.csv", data)
        for write, kw in ((write_plan_csv, {"context": ctx}), (write_plan_csv_host, {})):
            with pytest.raises(pd.errors.ParserError):
                write(src, str(tmp_path / "o.csv"), pc.CATS4, pc.FACTORS, labels=labels, **kw)
        assert not os.path.exists(tmp_path / "o.csv.part")
    else:
        dev, host, info = both(ctx, tmp_path, data, labels)
        same(dev, host)
        assert info["whole_file_fallback"] is True
    usable(ctx)


def test_chunking_gives_equal_bytes(ctx, tmp_path):
    n = 70000
    rows = rc.table_text(n, rc.HEADER11, seed=41, path=lambda i: f"/c/{i}")
    rows[99][0], rows[100][0], rows[65536][0] = "/a,b", '/c,d', "/e,f"  # a chunk's last and first rows
    data = rc.file_bytes(rc.HEADER11, rows)
    labels = pc.labels_for(n, 4, seed=6)
    dev, host, info = both(ctx, tmp_path, data, labels, chunk_rows=100)
    same(dev, host)
    assert info["deferred_rows"] == 3 and info["whole_file_fallback"] is False
    dev2, _, info = both(ctx, tmp_path, data, labels, chunk_rows=1 << 18)
    assert dev2 == dev and info["deferred_rows"] == 3


def usable(ctx):
    """The context still clusters: kmeans on the golden X equals the reference run."""
    import kmeans_plusplus as kp

    X = pd.read_csv(GOLDEN_CSV)[rc.FEATURES].values
    np.random.seed(0)
    C, labels = kp.kmeans(X, 4, number_of_files=len(X), random_state=42, context=ctx)
    ref = np.load(os.path.join(PDIR, "main_kmeans.npz"))
    np.testing.assert_array_equal(labels, ref["labels"])
    np.testing.assert_array_equal(C, ref["centroids"])


def test_error_paths_leave_the_context_usable(ctx, tmp_path):
    import _cdr

    data = pc.plain_file(50, seed=37)
    body = data.index(b"\n") + 1
    tails = pc.tails_of("abcd", [1, 2, 3, 4])
    labels = pc.labels_for(50, 4)
    bad = labels.copy()
    bad[17] = 4
    with pytest.raises(ValueError, match="label"):
        ctx.plan_format(data, body, 11, 0, bad, 4, tails)
    bad[17] = -1
    with pytest.raises(ValueError, match="label"):
        ctx.plan_format(data, body, 11, 0, bad, 4, tails)
    usable(ctx)
    with pytest.raises(ValueError, match="the file has 50 rows"):
        ctx.plan_format(data, body, 11, 0, labels[:49], 4, tails)
    with pytest.raises(ValueError, match="50 labels, the file has 51 rows"):  # the resident labels
        ctx.plan_format(pc.plain_file(51), body, 11, 0, None, 4, tails)
    usable(ctx)
    fresh = _cdr.Context(ctx.device)
    try:
        with pytest.raises(RuntimeError, match="no labels"):
            fresh.plan_format(data, body, 11, 0, None, 4, tails)
        with pytest.raises(RuntimeError, match="no labels"):
            fresh.plan_size_sums(np.zeros(0, dtype=np.int64), 4)
        with pytest.raises(RuntimeError, match="start at row 0"):
            fresh.plan_format(data, body, 11, 0, labels, 4, tails, row_begin=10)
    finally:
        fresh.close()
    with pytest.raises(ValueError, match="the rows need"):
        ctx.plan_format(data, body, 11, 0, labels, 4, tails, out=np.empty(100, dtype=np.uint8))
    # a short buffer keeps the index for the second call; an unsized call grows its own
    part = ctx.plan_format(data, body, 11, 0, labels, 4, tails, row_begin=10)
    part_text = part["text"].tobytes()  # (the context's buffer: valid until the next call)
    whole = ctx.plan_format(data, body, 11, 0, labels, 4, tails)["text"].tobytes()
    assert part["rows"] == 50 and whole.endswith(part_text)
    assert whole.count(b"\n") == 50 and part_text.count(b"\n") == 40
    bad[17] = 7  # a failed call of another kind drops it
    with pytest.raises(ValueError, match="label"):
        ctx.plan_format(data, body, 11, 0, bad, 4, tails)
    with pytest.raises(RuntimeError, match="start at row 0"):
        ctx.plan_format(data, body, 11, 0, labels, 4, tails, row_begin=10)
    with pytest.raises(ValueError):
        ctx.plan_format(data, body, 11, 11, labels, 4, tails)
    with pytest.raises(ValueError, match="tail"):
        ctx.plan_format(data, body, 11, 0, labels, 4, [b"," + b"x" * 64] * 4)
    with pytest.raises(NotImplementedError):
        ctx.plan_format(data, body, 11, 0, labels, 1025, [b",a,1\n"] * 1025)
    with pytest.raises(ValueError, match="negative size"):
        ctx.plan_size_sums([5, -1, 3], 4, [0, 1, 2])
    with pytest.raises(ValueError, match="label"):
        ctx.plan_size_sums([5, 1, 3], 2, [0, 1, 2])
    res = ctx.plan_format(data, body, 11, 0, labels, 4, tails)
    assert res["rows"] == 50 and res["deferred_rows"] == 0
    usable(ctx)


def test_resident_state_untouched(ctx, tmp_path):
    from features_csv import kmeans_csv
    from replication_plan import summarize, write_plan_csv

    t, cats = golden_tables()
    np.random.seed(0)
    C, _ = kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)

    step = ctx.lloyd_step_f64 if ctx.info()["mode"] == 2 else ctx.lloyd_step

    def state():
        return ctx.labels(), ctx.medians_by_label(4), step(C)

    before = state()
    write_plan_csv(GOLDEN_CSV, str(tmp_path / "p.csv"), cats, t["REPLICATION_FACTORS"], context=ctx)
    s = summarize(cats, t["REPLICATION_FACTORS"], 4, sizes=np.arange(50), current_factor=2, context=ctx)
    assert s["total"]["files"] == 50 and s["total"]["bytes"] == sum(range(50))
    after = state()
    for a, b in zip(before, after):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 300000])
@pytest.mark.parametrize("k", [1, 4, 1024])
def test_size_sums_against_python_ints(ctx, n, k):
    rng = np.random.default_rng(n + k)
    edge = np.array([0, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 62, 1], dtype=np.int64)
    sizes = np.where(rng.random(n) < 0.5, edge[rng.integers(0, len(edge), n)],
                     rng.integers(0, 2 ** 45, n)).astype(np.int64)
    sizes[0] = 2 ** 40
    labels = rng.integers(0, k, n).astype(np.int64)
    want = [0] * k
    for s, l in zip(sizes.tolist(), labels.tolist()):
        want[l] += s
    assert ctx.plan_size_sums(sizes, k, labels) == want


def test_size_sums_with_resident_labels(ctx):
    from features_csv import kmeans_csv

    np.random.seed(0)
    _, labels = kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)
    sizes = np.array([2 ** 40, 2 ** 32 - 1, 2 ** 32, 0] * 12 + [7, 9], dtype=np.int64)
    want = [sum(int(s) for s, l in zip(sizes, labels) if l == j) for j in range(4)]
    assert ctx.plan_size_sums(sizes, 4) == want
    assert ctx.plan_size_sums(sizes, 4, labels) == want
    with pytest.raises(ValueError):
        ctx.plan_size_sums(sizes[:49], 4)


def test_cli_end_to_end(ctx, tmp_path, capsys):
    import replication_plan

    t, cats = golden_tables()
    out = str(tmp_path / "plan.csv")
    np.random.seed(0)
    replication_plan.main(["--input_path", os.path.join(PDIR, "features_out"), "--k", "4",
                           "--tables", os.path.join(PDIR, "main_tables.json"), "--out", out,
                           "--manifest", os.path.join(PDIR, "metadata.csv"),
                           "--current_factor", "3"], context=ctx)
    plan = pd.read_csv(out)
    labels = np.load(os.path.join(PDIR, "main_kmeans.npz"))["labels"]
    assert list(plan["cluster"]) == list(labels)
    assert list(plan["category"]) == [cats[f"C{l}"] for l in labels]
    summary = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    assert sum(v["files"] for v in summary["categories"].values()) == 50
    total = int(pd.read_csv(os.path.join(PDIR, "metadata.csv"))["size_bytes"].sum())
    assert sum(v["bytes"] for v in summary["categories"].values()) == total
    assert summary["total"]["bytes"] == total and summary["total"]["files"] == 50


def test_a_failed_call_leaves_no_plan_file(ctx, tmp_path):
    from replication_plan import write_plan_csv

    src = pc.put(tmp_path / "f.csv", pc.plain_file(30))
    labels = pc.labels_for(30, 4)
    labels[11] = 4
    with pytest.raises(ValueError, match="label"):
        write_plan_csv(src, str(tmp_path / "o.csv"), pc.CATS4, pc.FACTORS, labels=labels, context=ctx)
    assert os.listdir(tmp_path) == ["f.csv"]


def test_the_text_buffer_grows_in_the_first_and_in_a_later_chunk(ctx, tmp_path):
    """Chunks of 10 rows start from 96 bytes per row: the 5000-byte path (chunk
    0) and the 65 535-byte one (row 255: the index is kept for the second call)."""
    rows = rc.table_text(300, rc.HEADER11, seed=43)
    rows[5][0], rows[255][0] = "/long/" + "p" * 5000, "y" * pc.MAX_FIELD
    dev, host, info = both(ctx, tmp_path, rc.file_bytes(rc.HEADER11, rows), pc.labels_for(300, 4),
                           chunk_rows=10)
    same(dev, host)
    clean(info, 300)


def test_resident_labels_are_checked_again_on_a_later_chunk(ctx, tmp_path):
    from features_csv import kmeans_csv

    np.random.seed(0)
    kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)
    data = pc.read(GOLDEN_CSV)
    body = data.index(b"\n") + 1
    tails = pc.tails_of("abcd", [1, 2, 3, 4])
    assert ctx.plan_format(data, body, 11, 0, None, 4, tails, 0, 10)["rows"] == 50
    assert ctx.plan_format(data, body, 11, 0, None, 4, tails, 10, 10)["text"].tobytes().count(b"\n") == 10
    ctx.load_points(np.random.default_rng(1).random((60, 5)))  # the labels are gone
    with pytest.raises(RuntimeError, match="no labels"):
        ctx.plan_format(data, body, 11, 0, None, 4, tails, 20, 10)
    usable(ctx)


def test_size_sums_without_sizes_count_the_rows(ctx):
    labels = pc.labels_for(5000, 7, seed=8)
    assert ctx.plan_size_sums(None, 7, labels) == np.bincount(labels, minlength=7).tolist()


def test_cli_takes_the_data_medians_without_global_medians(ctx, tmp_path, capsys):
    import replication_plan
    from features_csv import CLUSTERING_FEATURES
    from scoring import ClusterClassifier

    t, _ = golden_tables()
    del t["GLOBAL_MEDIANS"]
    tables = str(tmp_path / "tables.json")
    with open(tables, "w") as fh:
        json.dump(t, fh)
    out = str(tmp_path / "plan.csv")
    np.random.seed(0)
    replication_plan.main(["--input_path", GOLDEN_CSV, "--k", "4", "--tables", tables, "--out", out],
                          context=ctx)
    clf = ClusterClassifier.from_points(t["WEIGHTS"], t["DIRECTIONS"], t["REPLICATION_FACTORS"],
                                        CLUSTERING_FEATURES, context=ctx)
    cats = clf.classify_labels(4, CLUSTERING_FEATURES, context=ctx)
    X = pd.read_csv(GOLDEN_CSV)[CLUSTERING_FEATURES]
    assert clf.global_medians == {f: float(np.median(X[f])) for f in CLUSTERING_FEATURES}
    plan = pd.read_csv(out)
    labels = np.load(os.path.join(PDIR, "main_kmeans.npz"))["labels"]
    assert list(plan["cluster"]) == list(labels)
    assert list(plan["category"]) == [cats[f"C{l}"] for l in labels]
    assert list(plan["replication"]) == [t["REPLICATION_FACTORS"][cats[f"C{l}"]] for l in labels]

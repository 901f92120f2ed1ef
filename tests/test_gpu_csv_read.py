"""The features CSV read on the device (csrc/csvin.hip, features_csv.py) gives
the bits of pd.read_csv(path)[columns].values.  Expected values: pandas only."""
import glob
import io
import os
import random

import numpy as np
import pandas as pd
import pytest

import csv_cases as cc
import csv_read_cases as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")
GOLDEN_CSV = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
TILE = 4096          # bytes per tile of the record index (csvin.hip kTile)
STAGE = 16384        # LDS bytes staged per 64 rows (kStage)
SCAN_PART = 4096     # tiles per workgroup of the scan (kScanPart): 16 MiB of file
ROW_PAD = 8192       # rows are padded to a multiple of this (kSeedBlock)

# deferred cells pandas still reads as a number or NaN
NUMERIC_DEFER = [" 1.5", "1.5 ", "\t2", "NaN", "nan", "NA", "null", "NULL", "N/A", "inf", "-inf",
                 "Infinity", "-Infinity", "1234567890123456", "-9223372036854775808", "-0", "-000",
                 "1e-309", "0.0001e-305", "4.9e-324", "1e-400"]
# deferred cells that make pandas keep the column as text
TEXT_DEFER = ["1e", "1.5E", "2e+", ".", "-", "e5", "1.2.3", "1x", "0x10", "--1", "1e5.0", "1e309"]


def read(ctx, tmp_path, data, columns, name="f.csv"):
    from features_csv import read_features

    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    info = {}
    X = read_features(path, columns, ctx=ctx, info=info)
    return X, info


def same_bits(X, data, columns):
    want = rc.pandas_x(data, columns)
    assert X.dtype == np.float64 and X.shape == want.shape, (X.shape, want.shape)
    bad = np.argwhere(rc.bits_array(X) != rc.bits_array(want))
    assert bad.size == 0, (bad[:5], [X[tuple(b)] for b in bad[:5]], [want[tuple(b)] for b in bad[:5]])


def clean(info, rows):
    assert info["rows"] == rows and info["deferred_rows"] == 0, info
    assert not info["whole_file_fallback"] and info["resident"], info


def test_golden_pipeline_file(ctx):
    from features_csv import read_features

    info = {}
    X = read_features(GOLDEN_CSV, ctx=ctx, info=info)
    with open(GOLDEN_CSV, "rb") as fh:
        same_bits(X, fh.read(), rc.FEATURES)
    clean(info, len(X))
    assert all(k in info for k in ("upload_ms", "index_ms", "parse_ms", "finish_ms"))


def test_device_writer_output_over_the_writer_range(ctx, tmp_path):
    from compute_features import OUT_COLUMNS, write_spark_csv_device

    vals = [v for v in cc.double_cases()[0] if v == v and abs(v) != float("inf") and cc.in_device_range(v)]
    rows = len(vals) // 8
    table = np.zeros((rows, 10))
    table[:, [1, 2, 3, 5, 6, 7, 8, 9]] = np.array(vals[:rows * 8]).reshape(rows, 8)
    table[:, 0] = np.arange(rows) % 5000  # the long columns: counts
    table[:, 4] = np.arange(rows) % 64
    paths = cc.feature_paths(rows)
    paths[5], paths[77] = "/plain space", "/semi;colon"
    part = write_spark_csv_device(str(tmp_path / "out"), paths, table, ctx=ctx)
    with open(part, "rb") as fh:
        data = fh.read()
    from features_csv import read_features

    info = {}
    cols = OUT_COLUMNS[1:]
    X = read_features(part, cols, ctx=ctx, info=info)
    same_bits(X, data, cols)
    clean(info, rows)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, ROW_PAD + 1])
def test_row_counts(ctx, tmp_path, n_rows):
    rows = rc.table_text(n_rows, rc.HEADER11, seed=100 + n_rows)
    data = rc.file_bytes(rc.HEADER11, rows)
    X, info = read(ctx, tmp_path, data, rc.FEATURES)
    same_bits(X, data, rc.FEATURES)
    clean(info, n_rows)


@pytest.mark.parametrize("n_cols,d", [(11, 1), (11, 5), (17, 16), (20, 16), (20, 5), (1, 1)])
def test_column_selections_out_of_order(ctx, tmp_path, n_cols, d):
    rng = random.Random(n_cols * 100 + d)
    names = [f"c{j}" for j in range(n_cols)]
    n_rows = 300
    if n_cols == 1:  # one column: the cells alone
        rows = [[rc.numeric_text(rng, 0.5 if i == 0 else None)] for i in range(n_rows)]
        sel = [0]
    else:
        rows = rc.table_text(n_rows, names, seed=n_cols + d)
        sel = rng.sample(range(1, n_cols), d)
    cols = [names[j] for j in sel]
    data = rc.file_bytes(names, rows)
    X, info = read(ctx, tmp_path, data, cols)
    same_bits(X, data, cols)
    clean(info, n_rows)


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
    X, info = read(ctx, tmp_path, data, rc.FEATURES)
    same_bits(X, data, rc.FEATURES)
    clean(info, 200)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("shift", [0, 1, 2, 7])
def test_rows_at_the_tile_edge(ctx, tmp_path, eol, shift):
    """shift 0: a row's last byte is the last byte of a tile (for CRLF the '\\r'
    is, and its '\\n' opens the next tile); larger shifts straddle the edge."""
    rows = rc.table_text(120, rc.HEADER11, seed=11)
    header = ",".join(rc.HEADER11).encode() + eol
    lens = np.cumsum([len(",".join(r).encode()) + len(eol) for r in rows])
    j = int(np.searchsorted(lens, TILE)) + 1      # this row ends past the edge: move it onto it
    target = TILE + shift + (1 if eol == b"\r\n" and shift == 0 else 0)
    grow = target + TILE - int(lens[j])           # (one tile further: paths only grow)
    rows[j][0] += "x" * grow
    data = rc.file_bytes(rc.HEADER11, rows, eol=eol)
    body = data[len(header):]
    end = len(eol.join(",".join(r).encode() for r in rows[:j + 1])) + len(eol)
    assert end == 2 * TILE + shift + (1 if eol == b"\r\n" and shift == 0 else 0)
    assert body[end - 1:end] == b"\n"
    X, info = read(ctx, tmp_path, data, rc.FEATURES)
    same_bits(X, data, rc.FEATURES)
    clean(info, 120)


def test_a_row_longer_than_the_stage(ctx, tmp_path):
    rows = rc.table_text(130, rc.HEADER11, seed=13)
    rows[70][0] = "/long/" + "p" * (STAGE + 100)
    rows[129][0] = "/long/" + "q" * (3 * STAGE)
    data = rc.file_bytes(rc.HEADER11, rows)
    X, info = read(ctx, tmp_path, data, rc.FEATURES)
    same_bits(X, data, rc.FEATURES)
    clean(info, 130)


def test_more_than_one_scan_part(ctx, tmp_path):
    """Just over 16 MiB of short rows: the tile scan and the deferred-row scan
    run over several parts, the parse workgroups loop, and quotes far apart
    carry their parity across parts."""
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
    assert len(data) > SCAN_PART * TILE
    X, info = read(ctx, tmp_path, data, ["v"])
    same_bits(X, data, ["v"])
    assert info["rows"] == reps * len(block) + 3 and info["deferred_rows"] == 3
    assert not info["whole_file_fallback"]
    assert [float(X[m, 0]) for m in marks] == [0.25, 0.5, 0.75]


def mixed_file(cells, seed):
    """A 400-row file with one special cell (or path) per marked row."""
    rows = rc.table_text(400, rc.HEADER11, seed=seed)
    rng = random.Random(seed)
    marked = sorted(rng.sample(range(400), len(cells)))
    for r, c in zip(marked, cells):
        rows[r][6 + rng.randrange(5)] = c
    return rows, marked


def test_numeric_cells_of_every_defer_kind(ctx, tmp_path):
    rows, marked = mixed_file(NUMERIC_DEFER, seed=19)
    data = rc.file_bytes(rc.HEADER11, rows)
    X, info = read(ctx, tmp_path, data, rc.FEATURES)
    same_bits(X, data, rc.FEATURES)
    assert info["rows"] == 400 and info["deferred_rows"] == len(marked), info
    assert not info["whole_file_fallback"]
    assert not info["resident"]  # NaN and inf cells: load_points refuses such points too
    body = data[data.index(b"\n") + 1:]
    records, guard = rc.split_records(body)
    assert guard == -1
    got = [i for i, (b0, b1) in enumerate(records) if rc.row_is_deferred(body[b0:b1], 11, range(6, 11))]
    assert got == marked


def test_deferred_rows_are_exactly_the_injected_ones(ctx, tmp_path):
    """Quoted paths, short rows, an empty cell and finite deferred cells."""
    from features_csv import read_features

    rows = rc.table_text(500, rc.HEADER11, seed=23)
    special = {3: "/a,b", 64: '/q"uote', 65: "/two\nlines", 130: 'x,"y"\n,z', 131: '""', 499: "/last,one"}
    for r, p in special.items():
        rows[r][0] = p
    rows[200] = rows[200][:9]        # short: pandas fills NaN
    rows[301][8] = " 0.5"
    rows[302][7] = "12345678901234567"
    rows[303][10] = "-0"
    rows[304][6] = "1e-320"
    data = rc.file_bytes(rc.HEADER11, rows)
    marked = sorted(list(special) + [200, 301, 302, 303, 304])
    path = str(tmp_path / "m.csv")
    with open(path, "wb") as fh:
        fh.write(data)
    res = None
    with open(path, "rb") as fh:
        raw = fh.read()
    res = ctx.csv_read(raw, raw.index(b"\n") + 1, 11, list(range(6, 11)))
    assert res["deferred"][:, 0].tolist() == marked and res["guard"] == -1
    for r, b0, b1 in res["deferred"]:
        assert raw[b0:b1] == ",".join([rc.quote_path(rows[r][0])] + rows[r][1:]).encode()
    # the kinds: every shaped row's cells, per column
    kinds = res["col_kinds"]
    shaped = 500 - len(special) - 1
    assert (kinds.sum(axis=1) == shaped).all(), kinds
    assert kinds[:, rc.DEFER].tolist() == [1, 1, 1, 0, 1] and (kinds[:, rc.EMPTY] == 0).all()
    info = {}
    X = read_features(path, ctx=ctx, info=info)
    same_bits(X, data, rc.FEATURES)
    assert info["deferred_rows"] == len(marked) and not info["whole_file_fallback"]
    assert not info["resident"]  # the short row's NaN


def test_empty_cells_are_nan_on_the_device(ctx, tmp_path):
    rows = rc.table_text(100, rc.HEADER11, seed=29)
    rows[10][7] = ""
    rows[99][10] = ""
    data = rc.file_bytes(rc.HEADER11, rows)
    X, info = read(ctx, tmp_path, data, rc.FEATURES)
    same_bits(X, data, rc.FEATURES)
    assert info["deferred_rows"] == 0 and not info["whole_file_fallback"] and not info["resident"]


def test_int_columns(ctx, tmp_path):
    """A column pandas types int64: the deferred 17-digit cell is converted with
    one rounding; the same cell in a float column takes the float parser."""
    names = ["p", "a", "b"]
    rows = [[f"/f{i}", str(i * 7), rc.java_text(i / 7).decode()] for i in range(200)]
    rows[40][1] = "12345678901234567"
    rows[41][2] = "12345678901234567"
    rows[42][1] = "-0"
    data = rc.file_bytes(names, rows)
    X, info = read(ctx, tmp_path, data, ["b", "a"])
    same_bits(X, data, ["b", "a"])
    assert info["deferred_rows"] == 3 and not info["whole_file_fallback"] and info["resident"]
    rows[42][1] = "5"
    rows[43][1] = "9223372036854775808"  # past int64: pandas alone decides the column (uint64)
    data = rc.file_bytes(names, rows)
    assert pd.read_csv(io.BytesIO(data))["a"].dtype == np.uint64
    X, info = read(ctx, tmp_path, data, ["b", "a"])
    same_bits(X, data, ["b", "a"])
    assert info["whole_file_fallback"]


GUARDS = [(b'/a"b', 2), (b'"a"x', 2), (b' "q"', 1)]  # (path text, offset of the quote)


@pytest.mark.parametrize("case", range(5))
def test_guard_offsets_and_the_whole_file_path(ctx, tmp_path, case):
    rows = rc.table_text(150, rc.HEADER11, seed=31)
    data = rc.file_bytes(rc.HEADER11, rows)
    lines = data.split(b"\n")
    at = sum(len(ln) + 1 for ln in lines[:101])  # file offset of data row 100
    if case < 3:
        raw, off = GUARDS[case]
        lines[101] = raw + lines[101][lines[101].index(b","):]
    elif case == 3:
        lines[101:101] = [b" \t "]
        off = 0
    else:
        lines[101] = b'"open' + lines[101][lines[101].index(b","):]
        off = 0
    data = b"\n".join(lines)
    path = str(tmp_path / "g.csv")
    with open(path, "wb") as fh:
        fh.write(data)
    res = ctx.csv_read(data, data.index(b"\n") + 1, 11, list(range(6, 11)))
    assert res["guard"] == at + off, (res["guard"], at, off)
    from features_csv import read_features

    info = {}
    if case == 4:
        with pytest.raises(pd.errors.ParserError):
            read_features(path, ctx=ctx, info=info)
    else:
        X = read_features(path, ctx=ctx, info=info)
        same_bits(X, data, rc.FEATURES)
        assert info["whole_file_fallback"] and info["rows"] == len(X)
    usable(ctx)


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
    from features_csv import read_features

    rows = rc.table_text(50, rc.HEADER11, seed=37)
    data = rc.file_bytes(rc.HEADER11, rows)
    path = str(tmp_path / "e.csv")

    def put(d):
        with open(path, "wb") as fh:
            fh.write(d)

    put(data)
    with pytest.raises(KeyError) as e:
        read_features(path, ["age_norm", "nope"], ctx=ctx)
    with pytest.raises(KeyError) as want:
        pd.read_csv(path)[["age_norm", "nope"]]
    assert str(e.value) == str(want.value)
    usable(ctx)
    for cell in TEXT_DEFER:
        bad = [list(r) for r in rows]
        bad[20][7] = cell
        put(rc.file_bytes(rc.HEADER11, bad))
        assert pd.read_csv(path)["age_norm"].dtype == object, cell
        with pytest.raises(ValueError, match="age_norm"):
            read_features(path, ctx=ctx)
    usable(ctx)
    wide = [list(r) for r in rows]
    wide[30] = wide[30] + ["1", "2"]
    put(rc.file_bytes(rc.HEADER11, wide))
    with pytest.raises(pd.errors.ParserError):
        read_features(path, ctx=ctx)
    usable(ctx)
    with pytest.raises(RuntimeError):  # a finish without a read
        ctx.csv_read_finish(np.zeros(0, dtype=np.int64), np.zeros((0, 5)))
    with pytest.raises(NotImplementedError):
        ctx.csv_read(data, data.index(b"\n") + 1, 11, list(range(17)))
    with pytest.raises(ValueError):
        ctx.csv_read(data, data.index(b"\n") + 1, 11, [6, 6])
    with pytest.raises(ValueError):
        ctx.csv_read(data, data.index(b"\n") + 1, 11, [11])
    res = ctx.csv_read(data, data.index(b"\n") + 1, 11, [6, 7])
    with pytest.raises(ValueError):
        ctx.csv_read_finish([50], np.zeros((1, 2)))
    usable(ctx)


def test_points_state_equals_load_points(ctx, tmp_path):
    from features_csv import read_features

    # the golden file (fp64 values) and a file on an fp32 grid (F32X)
    grid = [[f"/g{i}"] + [repr(((i * 37 + j * 11) % 1024) / 1024.0) for j in range(10)] for i in range(3000)]
    for data in (open(GOLDEN_CSV, "rb").read(), rc.file_bytes(rc.HEADER11, grid)):
        path = str(tmp_path / "s.csv")
        with open(path, "wb") as fh:
            fh.write(data)
        X = read_features(path, ctx=ctx)
        got = ctx.info()
        rows = ctx.get_rows(np.arange(len(X)))
        np.testing.assert_array_equal(rc.bits_array(rows), rc.bits_array(X))
        ctx.load_points(X)
        assert ctx.info() == got
    assert got["mode"] == 1  # the grid file is F32X


def test_kmeans_csv_end_to_end(ctx):
    import json

    import kmeans_plusplus as kp
    from features_csv import kmeans_csv
    from scoring import ClusterClassifier

    X = pd.read_csv(GOLDEN_CSV)[rc.FEATURES].values
    np.random.seed(0)
    C0, lab0 = kp.kmeans(X, 4, number_of_files=len(X), random_state=42, context=ctx)
    np.random.seed(0)
    C, labels = kmeans_csv(GOLDEN_CSV, 4, random_state=42, context=ctx)
    np.testing.assert_array_equal(labels, lab0)
    np.testing.assert_array_equal(rc.bits_array(C), rc.bits_array(C0))
    with open(os.path.join(PDIR, "main_tables.json")) as fh:
        t = json.load(fh)
    clf = ClusterClassifier(t["GLOBAL_MEDIANS"], t["WEIGHTS"], t["DIRECTIONS"],
                            t["REPLICATION_FACTORS"], context=ctx)
    cats = clf.classify_labels(4, rc.FEATURES)
    final = pd.read_csv(os.path.join(PDIR, "final_categories.csv"), float_precision="round_trip")
    assert [cats[f"C{i}"] for i in range(4)] == list(final["category"])
    np.testing.assert_array_equal(C, final[rc.FEATURES].to_numpy())


def test_kmeans_csv_keeps_the_reference_iteration_rule(ctx, tmp_path):
    from features_csv import kmeans_csv

    rows = rc.table_text(10001, rc.HEADER11, seed=41)
    path = str(tmp_path / "big.csv")
    with open(path, "wb") as fh:
        fh.write(rc.file_bytes(rc.HEADER11, rows))
    with pytest.raises(TypeError):  # max(100, 10001 / 100) is a float (kmeans_plusplus.py:29-31)
        kmeans_csv(path, 4, random_state=1, context=ctx)
    C, labels = kmeans_csv(path, 4, random_state=1, max_iter=3, context=ctx)
    assert C.shape == (4, 5) and labels.shape == (10001,)

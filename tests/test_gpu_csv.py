"""The features CSV formatted on the device (csrc/csvout.hip) equals the host
writer's bytes.  Expected text: compute_features' host code only."""
import glob
import os

import numpy as np
import pandas as pd
import pytest

import csv_cases as cc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PDIR = os.path.join(GOLDEN, "pipeline")
LONG10 = (0, 4)  # access_freq and concurrency among OUT_COLUMNS[1:]

# Shape edges of csvout.hip: a workgroup of the row kernels covers 256 rows
# (kCsvBlock), the 256 threads of csv_scan_top take one workgroup sum each up to
# 256 * 256 = 65536 rows and several beyond; csv_cells and csv_emit put 256 cells
# or fields in a workgroup, which the row counts below cross at 10 columns too.
ROW_COUNTS = [1, 255, 256, 257, 1000]
MANY_ROWS = 80000  # > 65536: more than one workgroup sum per csv_scan_top thread

TRICKY = ["", None, "/a,b", '/a"b', "/a\nb", 'x,"y"\n,z', "/data/€中", "/long/" + "p" * 4093,
          '"""', "/cr\rx", "/nul\0x"]
assert len(TRICKY[7].encode()) == 4099


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def deferred_path(p):
    return p is not None and ("\r" in p or "\0" in p)


def expect(rows_text, is_deferred):
    """Body and deferred list of rows whose host text is rows_text."""
    body, deferred, off = [], [], 0
    for i, (txt, d) in enumerate(zip(rows_text, is_deferred)):
        if d:
            deferred.append((i, off))
        else:
            body.append(txt)
            off += len(txt)
    return b"".join(body), np.array(deferred, dtype=np.int64).reshape(-1, 2)


def rows_of_cells(paths, texts, n_cols):
    return [(p + "," + ",".join(texts[i * n_cols:(i + 1) * n_cols]) + "\n").encode()
            for i, p in enumerate(paths)]


def test_cell_parity_on_the_host_test_values(ctx):
    vals, exp = cc.double_cases()
    inside = [(v, e) for v, e in zip(vals, exp) if e is not None]
    inside += [(1.0, "1.0")] * (-len(inside) % 4)
    table = np.array([v for v, _ in inside]).reshape(-1, 4)
    paths = [f"p{i}" for i in range(len(table))]
    text, deferred = ctx.csv_format(table, paths, ())
    want = b"".join(rows_of_cells(paths, [e for _, e in inside], 4))
    assert len(deferred) == 0
    assert text.tobytes() == want


def test_out_of_range_cells_defer_their_rows(ctx):
    vals, exp = cc.double_cases()
    inside = [(v, e) for v, e in zip(vals, exp) if e is not None][:1000]
    table = np.array([v for v, _ in inside]).reshape(-1, 4)
    texts = [e for _, e in inside]
    paths = [f"p{i}" for i in range(len(table))]
    rows = rows_of_cells(paths, texts, 4)
    at = {0: 0, 17: 3, 100: 1, 101: 2, 249: 3, 130: 0}  # row -> column of the outside value
    outside = cc.OUTSIDE + [-cc.OUTSIDE[1], -5e-324]
    for (r, c), v in zip(sorted(at.items()), outside):
        table[r, c] = v
    want, want_def = expect(rows, [i in at for i in range(len(rows))])
    text, deferred = ctx.csv_format(table, paths, ())
    np.testing.assert_array_equal(deferred, want_def)
    assert text.tobytes() == want


@pytest.mark.parametrize("n_cols,long_cols", [(1, ()), (1, (0,)), (16, ()), (16, (0,)), (16, (15,)),
                                              (16, (0, 15))])
def test_column_counts_and_long_columns(ctx, n_cols, long_cols):
    rng = np.random.default_rng(3)
    n = 300
    table = np.array(cc.feature_values(n * n_cols, seed=5)[:n * n_cols]).reshape(n, n_cols)
    longs = np.array(cc.LONGS + [-v for v in cc.LONGS] + [123456789012.0, -0.5, 1e18])
    for j in long_cols:
        table[:, j] = np.where(rng.random(n) < 0.5, rng.integers(-10 ** 12, 10 ** 12, n) / 8.0,
                               longs[rng.integers(0, len(longs), n)])
    deferred_rows = {}
    if long_cols:
        for r, v in zip((5, 256, 299), cc.LONGS_DEFERRED + [float("-inf")]):
            table[r, long_cols[-1]] = v
            deferred_rows[r] = True
    paths = [f"/f/{i}" for i in range(n)]
    keep = [i for i in range(n) if i not in deferred_rows]
    host = dict(zip(keep, cc.host_rows([paths[i] for i in keep], table[keep], long_cols)))
    want, want_def = expect([host.get(i, b"") for i in range(n)], [i in deferred_rows for i in range(n)])
    text, deferred = ctx.csv_format(table, paths, long_cols)
    np.testing.assert_array_equal(deferred, want_def)
    assert text.tobytes() == want


@pytest.fixture(scope="module")
def tricky_rows():
    n = max(ROW_COUNTS)
    paths = [TRICKY[i % 16] if i % 16 < len(TRICKY) else f"/plain/{i}" for i in range(n)]
    paths[0] = "/first"
    table = cc.feature_table(n, seed=13)
    is_def = [deferred_path(p) for p in paths]
    keep = [i for i in range(n) if not is_def[i]]
    host = dict(zip(keep, cc.host_rows([paths[i] for i in keep], table[keep], LONG10)))
    return paths, table, [host.get(i, b"") for i in range(n)], is_def


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_rows_and_paths(ctx, tricky_rows, n):
    paths, table, rows, is_def = tricky_rows
    want, want_def = expect(rows[:n], is_def[:n])
    text, deferred = ctx.csv_format(table[:n], paths[:n], LONG10)
    np.testing.assert_array_equal(deferred, want_def)
    assert text.tobytes() == want


def test_each_tricky_path_alone(ctx):
    table = cc.feature_table(len(TRICKY), seed=17)
    for i, p in enumerate(TRICKY):
        text, deferred = ctx.csv_format(table[i:i + 1], [p], LONG10)
        if deferred_path(p):
            assert text.size == 0 and deferred.tolist() == [[0, 0]], p
        else:
            assert text.tobytes() == cc.host_rows([p], table[i:i + 1], LONG10)[0], p
            assert len(deferred) == 0


@pytest.fixture(scope="module")
def tiled():
    n = 2000
    table, paths = cc.feature_table(n, seed=19), cc.feature_paths(n)
    paths[7], paths[1999] = 'q"uote,d', ""
    body = b"".join(cc.host_rows(paths, table, LONG10))
    reps = MANY_ROWS // n
    return np.tile(table, (reps, 1)), paths * reps, body * reps


def test_scan_over_many_workgroups(ctx, tiled):
    table, paths, body = tiled
    assert len(paths) == MANY_ROWS
    text, deferred = ctx.csv_format(table, paths, LONG10)
    assert len(deferred) == 0
    assert text.tobytes() == body


def test_device_writer_with_chunk_edges_inside_the_table(ctx, tiled, tmp_path):
    from compute_features import OUT_COLUMNS, write_spark_csv_device

    table, paths, body = tiled
    part = write_spark_csv_device(str(tmp_path / "out"), paths, table, ctx=ctx, chunk_rows=30011)
    assert read(part) == (",".join(OUT_COLUMNS) + "\n").encode() + body
    assert ctx.last_csv == {"rows": MANY_ROWS, "deferred": 0, "bytes": os.path.getsize(part)}
    assert os.path.exists(tmp_path / "out" / "_SUCCESS")


def test_pipeline_golden_and_synthetic_without_deferral(ctx, tmp_path):
    from compute_features import write_spark_csv, write_spark_csv_device

    golden = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
    z = np.load(os.path.join(PDIR, "features_oracle.npz"))
    paths = list(pd.read_csv(golden)["path"])
    part = write_spark_csv_device(str(tmp_path / "g"), paths, z["table"], ctx=ctx)
    assert read(part) == read(golden)
    assert ctx.last_csv["deferred"] == 0 and ctx.last_csv["rows"] == len(paths)
    n = 5000
    table, paths = cc.feature_table(n, seed=23), cc.feature_paths(n)
    part = write_spark_csv_device(str(tmp_path / "s"), paths, table, ctx=ctx)
    assert read(part) == read(write_spark_csv(str(tmp_path / "h"), paths, table))
    assert ctx.last_csv["deferred"] == 0 and ctx.last_csv["rows"] == n


def test_main_keeps_the_host_writer_for_jdk19_digits(ctx, tmp_path, monkeypatch):
    import compute_features as cf

    def no_device_writer(*a, **k):
        raise AssertionError("the device writer has the pre-19 digits only")

    monkeypatch.setenv("CDR_JAVA_DOUBLE", "19")
    monkeypatch.setattr(cf, "write_spark_csv_device", no_device_writer)
    out = tmp_path / "features_out"
    cf.main(["--manifest", os.path.join(PDIR, "metadata.csv"),
             "--access_log", os.path.join(PDIR, "access.log"), "--out", str(out)])
    got = read(glob.glob(str(out / "part-00000*.csv"))[0])
    z = np.load(os.path.join(PDIR, "features_oracle.npz"))
    golden = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]
    want = cf.write_spark_csv(str(tmp_path / "h"), list(pd.read_csv(golden)["path"]), z["table"],
                              fmt=cf.java_double)
    assert got == read(want)


def test_errors_leave_the_context_usable(ctx):
    table, paths = cc.feature_table(50, seed=29), cc.feature_paths(50)
    for n_cols in (0, 17):
        with pytest.raises(NotImplementedError):
            ctx.csv_format(np.zeros((3, n_cols)), ["a", "b", "c"], ())
    want = b"".join(cc.host_rows(paths, table, LONG10))
    with pytest.raises(ValueError):
        ctx.csv_format(table, paths, LONG10, cap=len(want) - 1)
    with pytest.raises(ValueError):
        ctx.csv_format(table, paths[:-1], LONG10)
    text, deferred = ctx.csv_format(table, paths, LONG10, cap=len(want))
    assert text.tobytes() == want and len(deferred) == 0
    text, deferred = ctx.csv_format(np.zeros((0, 10)), [], LONG10)
    assert text.size == 0 and deferred.shape == (0, 2)

"""write_spark_csv_device's chunking and splice of deferred rows, against
write_spark_csv, with a fake context built from the host formatter (CPU)."""
import csv
import os

import numpy as np
import pytest

import csv_cases as cc


class FakeCtx:
    """csv_format as the device gives it, formatted by the host code; the rows
    whose path is in `defer` are deferred: no bytes, listed as {row, offset}."""

    def __init__(self, defer=()):
        self.defer = set(defer)
        self.calls = []

    def csv_format(self, table, paths, long_cols=()):
        self.calls.append(len(paths))
        parts, deferred, off = [], [], 0
        for i, pth in enumerate(paths):
            if pth in self.defer:
                deferred.append((i, off))
                continue
            parts.append(cc.host_rows([pth], table[i:i + 1], tuple(long_cols))[0])
            off += len(parts[-1])
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        return text, np.array(deferred, dtype=np.int64).reshape(-1, 2)


N = 20
PATHS = [f"/d/f{i}" for i in range(N)]
PATHS[3], PATHS[4], PATHS[9] = 'a,"b"\nc', "", "/d/€"
TABLE = cc.feature_table(N)


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def host_file(tmp_path_factory):
    from compute_features import write_spark_csv

    return read(write_spark_csv(str(tmp_path_factory.mktemp("host") / "out"), PATHS, TABLE))


@pytest.mark.parametrize("defer", [[], [0], [N - 1], [7, 8], list(range(N))],
                         ids=["none", "first", "last", "adjacent", "all"])
@pytest.mark.parametrize("chunk", [1, 7, N, N + 1])
def test_device_writer_equals_host_writer(tmp_path, host_file, defer, chunk):
    from compute_features import write_spark_csv_device

    ctx = FakeCtx([PATHS[i] for i in defer])
    part = write_spark_csv_device(str(tmp_path / "out"), PATHS, TABLE, ctx=ctx, chunk_rows=chunk)
    assert read(part) == host_file
    assert ctx.calls == [min(chunk, N - lo) for lo in range(0, N, chunk)]
    assert ctx.last_csv == {"rows": N, "deferred": len(defer), "bytes": len(host_file)}


def test_no_rows_gives_the_header_only(tmp_path):
    from compute_features import OUT_COLUMNS, write_spark_csv, write_spark_csv_device

    ctx = FakeCtx()
    part = write_spark_csv_device(str(tmp_path / "dev"), [], np.zeros((0, 10)), ctx=ctx)
    assert read(part) == (",".join(OUT_COLUMNS) + "\n").encode()
    assert read(part) == read(write_spark_csv(str(tmp_path / "host"), [], np.zeros((0, 10))))
    assert ctx.calls == [] and ctx.last_csv["rows"] == 0


def test_overwrite_and_success_marker(tmp_path):
    from compute_features import write_spark_csv, write_spark_csv_device

    for name, write in (("dev", lambda d: write_spark_csv_device(d, PATHS, TABLE, ctx=FakeCtx())),
                        ("host", lambda d: write_spark_csv(d, PATHS, TABLE))):
        out = tmp_path / name
        out.mkdir()
        (out / "part-00000-old-c000.csv").write_text("stale")
        (out / "leftover").write_text("x")
        part = write(str(out))
        names = sorted(os.listdir(out))
        assert names == ["_SUCCESS", os.path.basename(part)], names
        assert os.path.basename(part).startswith("part-00000-") and part.endswith("-c000.csv")
        assert os.path.getsize(out / "_SUCCESS") == 0
    with pytest.raises(ValueError):
        write_spark_csv_device(str(tmp_path / "z"), PATHS, TABLE, ctx=FakeCtx(), chunk_rows=0)


def test_deferred_rows_raise_what_the_host_writer_raises(tmp_path):
    from compute_features import write_spark_csv, write_spark_csv_device

    paths = list(PATHS)
    paths[5] = "/d/nul\0"
    with pytest.raises(csv.Error):
        write_spark_csv(str(tmp_path / "h1"), paths, TABLE)
    with pytest.raises(csv.Error):
        write_spark_csv_device(str(tmp_path / "d1"), paths, TABLE, ctx=FakeCtx([paths[5]]))
    table = TABLE.copy()
    table[6, 0] = float("nan")  # access_freq is a long column
    with pytest.raises(ValueError):
        write_spark_csv(str(tmp_path / "h2"), PATHS, table)
    with pytest.raises(ValueError):
        write_spark_csv_device(str(tmp_path / "d2"), PATHS, table, ctx=FakeCtx([PATHS[6]]))

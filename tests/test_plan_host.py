"""The replication plan's definition (write_plan_csv_host), write_plan_csv's
chunking and splice over a host-backed context, and summarize (CPU)."""
import csv
import glob
import io
import json
import os
import re

import numpy as np
import pandas as pd
import pytest

import csv_read_cases as rc
import plan_cases as pc
from conftest import GOLDEN, PKG

PDIR = os.path.join(GOLDEN, "pipeline")
GOLDEN_CSV = glob.glob(os.path.join(PDIR, "features_out", "part-00000*.csv"))[0]


def test_host_writer_equals_pandas_to_csv_on_plain_paths(tmp_path):
    from replication_plan import write_plan_csv_host

    n = 300
    rows = rc.table_text(n, rc.HEADER11, seed=3)
    rows[5][0], rows[6][0], rows[7][0] = "/with space/and\ttab", "/données/ß€.bin", "x"
    src = pc.put(tmp_path / "f.csv", rc.file_bytes(rc.HEADER11, rows))
    labels = pc.labels_for(n, 4)
    info = {}
    got = write_plan_csv_host(src, str(tmp_path / "p.csv"), pc.CATS4, pc.FACTORS, labels=labels,
                              info=info)
    cats = [pc.CATS4[f"C{l}"] for l in labels]
    want = pd.DataFrame({"path": [r[0] for r in rows], "cluster": labels, "category": cats,
                         "replication": [pc.FACTORS[c] for c in cats]}).to_csv(index=False)
    assert got == n and pc.read(tmp_path / "p.csv") == want.encode("utf-8")
    assert info == {"rows": n, "deferred_rows": 0, "whole_file_fallback": True}


def test_golden_pipeline_plan(tmp_path):
    from replication_plan import write_plan_csv_host

    labels = np.load(os.path.join(PDIR, "main_kmeans.npz"))["labels"]
    final = pd.read_csv(os.path.join(PDIR, "final_categories.csv"))
    with open(os.path.join(PDIR, "main_tables.json")) as fh:
        factors = json.load(fh)["REPLICATION_FACTORS"]
    cats = {f"C{j}": c for j, c in enumerate(final["category"])}
    out = str(tmp_path / "plan.csv")
    assert write_plan_csv_host(GOLDEN_CSV, out, cats, factors, labels=labels) == 50
    assert len(pc.read(out).split(b"\n")) == 52  # 51 lines, each ended
    plan = pd.read_csv(out)
    assert list(plan.columns) == ["path", "cluster", "category", "replication"]
    assert list(plan["path"]) == list(pd.read_csv(GOLDEN_CSV)["path"])
    assert list(plan["cluster"]) == list(labels)
    assert list(plan["category"]) == [final["category"][l] for l in labels]
    assert list(plan["replication"]) == [factors[final["category"][l]] for l in labels]


N = 20


def splice_file():
    rows = rc.table_text(N, rc.HEADER11, seed=5)
    rows[3][0], rows[4][0], rows[9][0] = 'a,"b"\nc', "", "/d/€"
    rows[12] = rows[12] + ["extra"]        # ragged: deferred by the device's own rule
    return rc.file_bytes(rc.HEADER11, rows)


@pytest.mark.parametrize("defer", [[], [0], [N - 1], [6, 7], [0, 6, 7, 13, 14, N - 1]],
                         ids=["own", "first", "last", "chunk-edge", "many"])
@pytest.mark.parametrize("chunk", [1, 7, N])
@pytest.mark.parametrize("resident", [False, True])
def test_device_writer_equals_host_writer_over_a_fake_context(tmp_path, defer, chunk, resident):
    """chunk 7: rows 6, 7, 13 and 14 are a chunk's last and first rows."""
    from replication_plan import write_plan_csv, write_plan_csv_host

    src = pc.put(tmp_path / "f.csv", splice_file())
    labels = pc.labels_for(N, 4, seed=2)
    write_plan_csv_host(src, str(tmp_path / "host.csv"), pc.CATS4, pc.FACTORS, labels=labels)
    ctx = pc.FakeCtx(defer, resident=labels if resident else None)
    info = {}
    n = write_plan_csv(src, str(tmp_path / "dev.csv"), pc.CATS4, pc.FACTORS,
                       labels=None if resident else labels, context=ctx, chunk_rows=chunk,
                       info=info)
    assert pc.read(tmp_path / "dev.csv") == pc.read(tmp_path / "host.csv")
    assert ctx.calls == [(lo, min(chunk, N - lo)) for lo in range(0, N, chunk)]
    assert n == N and info["rows"] == N and info["whole_file_fallback"] is False
    assert info["deferred_rows"] == len(set(defer) | {3, 12})


def test_whole_file_cases_equal_the_host_writer(tmp_path):
    from replication_plan import write_plan_csv, write_plan_csv_host

    rows = rc.table_text(N, rc.HEADER11, seed=7)
    labels = pc.labels_for(N, 4)
    guard = [list(r) for r in rows]
    guard[8][0] = '/a"b'                          # a guard hit
    lone_cr = [list(r) for r in rows]
    lone_cr[8][0] = "/a\rb"                       # pandas splits the deferred row
    index = [list(r) for r in rows]
    index[0] = index[0] + ["1"]                   # the first row makes pandas infer an index
    files = [rc.file_bytes(rc.HEADER11, guard).replace(b'"/a""b"', b'/a"b'),
             rc.file_bytes(rc.HEADER11, lone_cr).replace(b'"/a\rb"', b"/a\rb"),
             rc.file_bytes(rc.HEADER11, index),
             b"\xef\xbb\xbf" + rc.file_bytes(rc.HEADER11, rows)]  # a header _header cannot take
    for i, data in enumerate(files):
        src = pc.put(tmp_path / f"f{i}.csv", data)
        lab = labels if i != 1 else np.append(labels, 0)  # (the lone CR makes one more row)
        info = {}
        write_plan_csv(src, str(tmp_path / "dev.csv"), pc.CATS4, pc.FACTORS, labels=lab,
                       context=pc.FakeCtx(), info=info, chunk_rows=7)
        write_plan_csv_host(src, str(tmp_path / "host.csv"), pc.CATS4, pc.FACTORS, labels=lab)
        assert pc.read(tmp_path / "dev.csv") == pc.read(tmp_path / "host.csv"), i
        assert info["whole_file_fallback"] is True, i
    # a tail longer than the table's slot
    cats = {"C0": "x" * 70}
    src = pc.put(tmp_path / "t.csv", rc.file_bytes(rc.HEADER11, rows))
    info = {}
    write_plan_csv(src, str(tmp_path / "dev.csv"), cats, {"x" * 70: 1}, labels=np.zeros(N, int),
                   context=pc.FakeCtx(), info=info)
    assert info["whole_file_fallback"] is True
    assert pc.read(tmp_path / "dev.csv").count(b"x" * 70) == N


def test_a_category_that_needs_quoting_is_quoted_by_the_host_once(tmp_path):
    from replication_plan import write_plan_csv, write_plan_csv_host

    cats = {"C0": 'Hot, "really"', "C1": "Cold"}
    factors = {'Hot, "really"': 0, "Cold": 125}
    src = pc.put(tmp_path / "f.csv", pc.plain_file(N))
    labels = pc.labels_for(N, 2)
    write_plan_csv_host(src, str(tmp_path / "host.csv"), cats, factors, labels=labels)
    write_plan_csv(src, str(tmp_path / "dev.csv"), cats, factors, labels=labels,
                   context=pc.FakeCtx())
    got = pc.read(tmp_path / "dev.csv")
    assert got == pc.read(tmp_path / "host.csv")
    rows = list(csv.reader(io.StringIO(got.decode())))[1:]
    assert [r[1:] for r in rows] == [[str(l)] + [['Hot, "really"', "0"], ["Cold", "125"]][l]
                                     for l in labels]


def test_table_errors(tmp_path):
    from replication_plan import summarize, write_plan_csv, write_plan_csv_host

    src = pc.put(tmp_path / "f.csv", pc.plain_file(4))
    lab = np.zeros(4, dtype=np.int64)
    for write, kw in ((write_plan_csv, {"context": pc.FakeCtx()}), (write_plan_csv_host, {})):
        with pytest.raises(ValueError, match="no category"):
            write(src, str(tmp_path / "o.csv"), {"C0": "Hot", "C2": "Hot"}, pc.FACTORS, labels=lab, **kw)
        with pytest.raises(ValueError, match="no replication factor"):
            write(src, str(tmp_path / "o.csv"), {"C0": "Warm"}, pc.FACTORS, labels=lab, **kw)
        for bad in (-1, 2.0, "3", True, None):
            with pytest.raises(ValueError, match="not an int"):
                write(src, str(tmp_path / "o.csv"), {"C0": "Hot"}, {"Hot": bad}, labels=lab, **kw)
    with pytest.raises(ValueError, match="no category"):  # a label past the categories
        write_plan_csv_host(src, str(tmp_path / "o.csv"), {"C0": "Hot"}, pc.FACTORS, labels=lab + 1)
    with pytest.raises(ValueError):
        write_plan_csv_host(src, str(tmp_path / "o.csv"), {"C0": "Hot"}, pc.FACTORS, labels=lab[:3])
    with pytest.raises(ValueError):
        write_plan_csv(src, str(tmp_path / "o.csv"), {"C0": "Hot"}, pc.FACTORS, labels=lab,
                       context=pc.FakeCtx(), chunk_rows=0)
    ctx = pc.FakeCtx()
    with pytest.raises(ValueError, match="no category"):
        summarize({"C0": "Hot"}, pc.FACTORS, 2, labels=lab, context=ctx)
    with pytest.raises(ValueError, match="no replication factor"):
        summarize({"C0": "Warm"}, pc.FACTORS, 1, labels=lab, context=ctx)
    with pytest.raises(ValueError, match="not an int"):
        summarize({"C0": "Hot"}, {"Hot": 1.5}, 1, labels=lab, context=ctx)
    with pytest.raises(ValueError, match="current_factor"):
        summarize({"C0": "Hot"}, pc.FACTORS, 1, labels=lab, context=ctx, sizes=lab, current_factor=-1)
    with pytest.raises(ValueError, match="sizes"):
        summarize({"C0": "Hot"}, pc.FACTORS, 1, labels=lab, context=ctx, sizes=lab[:2])


def test_summarize_against_python_ints():
    from replication_plan import summarize

    # clusters 0 and 3 are Moderate (1), 1 Hot (3), 2 Archival (4), 4 Shared (2) without files
    cats = dict(pc.CATS4, C3="Moderate", C4="Shared")
    labels = np.array([0, 1, 1, 2, 3, 3, 0, 2], dtype=np.int64)
    sizes = [2 ** 40, 2 ** 32 - 1, 2 ** 40, 0, 2 ** 32, 7, 2 ** 62, 2 ** 32 - 1]
    by = {"Moderate": sizes[0] + sizes[4] + sizes[5] + sizes[6], "Hot": sizes[1] + sizes[2],
          "Archival": sizes[3] + sizes[7], "Shared": 0}
    ctx = pc.FakeCtx(resident=labels)
    s = summarize(cats, pc.FACTORS, 5, labels=labels, context=ctx)
    assert {c: v["files"] for c, v in s["categories"].items()} == {"Moderate": 4, "Hot": 2, "Archival": 2, "Shared": 0}
    assert s["categories"]["Moderate"]["clusters"] == [0, 3] and s["total"] == {"files": 8}
    assert "bytes" not in s["categories"]["Hot"]
    for current in (0, 1, 2, 3, 4, 5):  # below, equal to and above the factors 1, 2, 3, 4
        s = summarize(cats, pc.FACTORS, 5, sizes=sizes, current_factor=current, context=ctx)
        for c, v in s["categories"].items():
            f = pc.FACTORS[c]
            assert v["factor"] == f and v["bytes"] == by[c] and v["replica_bytes"] == f * by[c]
            assert v["bytes_to_copy"] == max(f - current, 0) * by[c]
            assert v["bytes_to_free"] == max(current - f, 0) * by[c]
            assert all(type(v[key]) is int for key in ("files", "bytes", "replica_bytes"))
        assert s["total"]["bytes"] == sum(sizes)
        assert s["total"]["replica_bytes"] == sum(pc.FACTORS[c] * b for c, b in by.items())
        assert s["total"]["bytes_to_copy"] == sum(max(pc.FACTORS[c] - current, 0) * b for c, b in by.items())
    s = summarize(cats, pc.FACTORS, 5, sizes=sizes, context=ctx)
    assert "bytes_to_copy" not in s["total"] and s["total"]["bytes"] == sum(sizes)


def test_the_module_does_not_import_the_oracle():
    with open(os.path.join(PKG, "replication_plan.py")) as fh:
        assert not re.search(r"^\s*(from|import)\s+oracle", fh.read(), flags=re.M)


def test_an_error_or_a_fallback_leaves_no_partial_file(tmp_path):
    from replication_plan import write_plan_csv

    class Refusing(pc.FakeCtx):
        def plan_format(self, *a, **kw):
            if self.calls:
                raise ValueError("plan: label outside [0, k)")
            return super().plan_format(*a, **kw)

    src = pc.put(tmp_path / "f.csv", pc.plain_file(N))
    with pytest.raises(ValueError, match="label outside"):  # the second chunk's call fails
        write_plan_csv(src, str(tmp_path / "o.csv"), pc.CATS4, pc.FACTORS, labels=pc.labels_for(N, 4),
                       context=Refusing(), chunk_rows=7)
    assert os.listdir(tmp_path) == ["f.csv"]
    data = pc.plain_file(N).replace(b"/data/set08", b'/da"a/set08')  # a guard hit in the second chunk
    src = pc.put(tmp_path / "f.csv", data)
    info = {}
    write_plan_csv(src, str(tmp_path / "o.csv"), pc.CATS4, pc.FACTORS, labels=pc.labels_for(N, 4),
                   context=pc.FakeCtx(), chunk_rows=7, info=info)
    assert info["whole_file_fallback"] is True and sorted(os.listdir(tmp_path)) == ["f.csv", "o.csv"]

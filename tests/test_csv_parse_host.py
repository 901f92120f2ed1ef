"""csrc/csv_parse.h on the host: one cell parses to the bits pd.read_csv gives
(its default float parser is not correctly rounded), and the record index and
guard of csrc/csvin.hip, as a Python model, agree with pandas (CPU; the cell
check needs g++)."""
import io
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import csv_read_cases as rc
from conftest import REPO


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the host check of csv_parse.h cannot be built")
    exe = str(tmp_path_factory.mktemp("csvp") / "csv_parse_check")
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-std=c++17",
                    os.path.join(REPO, "tools", "csv_parse_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, texts):
    out = subprocess.run([exe], input=b"".join(t + b"\n" for t in texts), stdout=subprocess.PIPE,
                         check=True).stdout.split(b"\n")[:-1]
    assert len(out) == len(texts)
    kinds = np.array([int(line[:1]) for line in out])
    bits = np.array([int(line[2:], 16) for line in out], dtype=np.uint64)
    return kinds, bits


def test_float_cells_equal_pandas_bit_for_bit(checker):
    texts = rc.float_cells()
    assert len(texts) >= 200000
    want = rc.bits_array(rc.pandas_column(texts))
    kinds, bits = run(checker, texts)
    inf = np.isinf(want.view(np.float64))
    expect_kind = np.array([rc.expected_kind(t, bool(i)) for t, i in zip(texts, inf)])
    bad = np.flatnonzero(kinds != expect_kind)
    assert bad.size == 0, [(texts[i], kinds[i], expect_kind[i]) for i in bad[:10]]
    parsed = kinds != rc.DEFER
    assert parsed.sum() >= 200000
    diff = np.flatnonzero(parsed & (bits != want))
    assert diff.size == 0, [(texts[i], hex(bits[i]), hex(want[i])) for i in diff[:10]]
    # the cells where pandas is not the correctly rounded float(text): a
    # strtod-quality parser fails on every one of them
    exact = rc.bits_array(np.array([float(t) for t in texts]))
    off = parsed & (want != exact)
    assert off.sum() >= 1000, int(off.sum())
    # only out-of-range cells were deferred here, and some were
    deferred = [texts[i] for i in np.flatnonzero(~parsed)]
    assert 0 < len(deferred) < 1000
    assert all(b"e" in t.lower() for t in deferred)


def test_python_model_equals_the_header(checker):
    texts = rc.float_cells()[::7] + rc.int_cells() + [t.encode() for t in rc.DEFER_CELLS] + [b""]
    kinds, bits = run(checker, texts)
    for t, k, b in zip(texts, kinds, bits):
        mk, mv = rc.model_cell(t)
        assert mk == k, (t, mk, k)
        if mk != rc.DEFER:
            assert rc.bits_of(mv) == int(b), (t, mv, hex(b))


def test_int_cells_equal_the_int64_column(checker):
    texts = rc.int_cells()
    frame = pd.read_csv(io.BytesIO(b"x\n" + b"\n".join(texts) + b"\n"))
    assert frame["x"].dtype == np.int64
    want = rc.bits_array(frame["x"].values.astype(np.float64))
    kinds, bits = run(checker, texts)
    assert (kinds == rc.INT).all()
    assert (bits == want).all()
    # and the float path pandas takes when another cell of the column is a float
    as_float = rc.bits_array(rc.pandas_column(texts + [b"0.5"]))[:-1]
    assert (bits == as_float).all()


def test_defer_and_empty(checker):
    texts = [t.encode() for t in rc.DEFER_CELLS + rc.OVERFLOW_CELLS + rc.TOO_WIDE]
    kinds, _ = run(checker, texts)
    assert (kinds == rc.DEFER).all(), [t for t, k in zip(texts, kinds) if k != rc.DEFER]
    kinds, bits = run(checker, [b""])
    assert kinds[0] == rc.EMPTY and int(bits[0]) == rc.NAN_BITS
    assert rc.bits_of(pd.read_csv(io.BytesIO(b"a,b\n1,\n"))["b"].values[0]) == rc.NAN_BITS
    # "-0" is why an int-like negative zero is deferred: the column's type decides
    assert rc.bits_of(rc.pandas_column([b"-0", b"1"])[0]) == 0
    assert rc.bits_of(rc.pandas_column([b"-0", b"1.5"])[0]) == 1 << 63


# ---- the record index and the guard, as a model, against pandas -----------------------
def record_files():
    names = rc.HEADER11
    rows = rc.table_text(40, names, seed=3)
    rows[3][0] = "/a,b"
    rows[9][0] = '/q"uote'
    rows[17][0] = "/two\nlines"
    rows[18][0] = '/x,"y"\n,z'
    rows[30][0] = '""'
    plain = rc.table_text(40, names, seed=4)
    yield "quoted", rc.file_bytes(names, rows)
    yield "crlf", rc.file_bytes(names, rows, eol=b"\r\n")
    yield "no last newline", rc.file_bytes(names, plain, last_eol=False)
    yield "crlf no last newline", rc.file_bytes(names, plain, eol=b"\r\n", last_eol=False)
    data = rc.file_bytes(names, plain)
    lines = data.split(b"\n")
    yield "blank lines", b"\n".join(lines[:5] + [b"", b""] + lines[5:9] + [b"\r"] + lines[9:]) + b"\n\n"
    yield "one row", rc.file_bytes(names, plain[:1])


@pytest.mark.parametrize("name,data", list(record_files()), ids=lambda v: v if isinstance(v, str) else "")
def test_record_model_agrees_with_pandas(name, data):
    body_off = data.index(b"\n") + 1
    header, body = data[:body_off], data[body_off:]
    records, guard = rc.split_records(body)
    frame = pd.read_csv(io.BytesIO(data))
    assert guard == -1
    assert len(records) == len(frame)
    for i, (b0, b1) in enumerate(records):
        one = pd.read_csv(io.BytesIO(header + body[b0:b1] + b"\n"))
        assert len(one) == 1
        assert one.iloc[0]["path"] == frame.iloc[i]["path"]
        got, want = rc.bits_array(one[rc.FEATURES].values), rc.bits_array(frame.iloc[i:i + 1][rc.FEATURES].values)
        assert (got == want).all()


GUARD_FILES = [
    # (body, the offset in the body where the guard fires)
    (b'a"b,1\nc,2\n', 1),
    (b'x,1\n"a"x,1\nc,2\n', 6),
    (b'x,1\ny, "q",1\n', 7),
    (b'x,1\n  \t\ny,2\n', 4),
    (b'x,1\n"open,2\ny,3\n', 4),
    (b'x,1\ny,"a""b"z,2\n', 11),
]


@pytest.mark.parametrize("body,offset", GUARD_FILES)
def test_guard_model_fires_where_pandas_leaves_plain_parity(body, offset):
    assert rc.split_records(body)[1] == offset
    # ... and these are files on which the plain split is not pandas' (or pandas raises)
    data = b"k,v\n" + body
    try:
        frame = pd.read_csv(io.BytesIO(data))
    except pd.errors.ParserError:
        return
    records, _ = rc.split_records(body)
    keys = [body[b0:b1].split(b",")[0].decode() for b0, b1 in records]
    assert len(records) != len(frame) or keys != [str(k) for k in frame["k"]]


def test_well_formed_quotes_do_not_fire_the_guard():
    for body in (b'"a,b",1\n', b'"a""b",1\n"",2\n', b'x,"q"\r\n', b'"multi\nline",1\n', b'x,"end"'):
        assert rc.split_records(body)[1] == -1, body

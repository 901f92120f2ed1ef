"""Inputs of the features-CSV read tests, and Python models of what the device
does, so that the CPU suite can hold them against pandas.

The expected values always come from pandas (``pd.read_csv``), never from the
code under test.  ``model_cell`` restates csrc/csv_parse.h, ``expected_kind``
classifies a cell from its text alone (regular expressions and integer
arithmetic), ``split_records`` restates the record index and the guard of
csrc/csvin.hip."""
import functools
import io
import math
import random
import re
import struct

import numpy as np

INT, FLOAT, EMPTY, DEFER = 0, 1, 2, 3
NAN_BITS = 0x7FF8000000000000
FEATURES = ["access_freq_norm", "age_norm", "write_ratio_norm", "locality_norm", "concurrency_norm"]
HEADER11 = ["path", "access_freq", "age_seconds", "write_ratio", "locality", "concurrency"] + FEATURES

# every cell of a DEFER kind (csv_parse.h), as text
DEFER_CELLS = [" 1.5", "1.5 ", "\t2", "NaN", "nan", "Infinity", "-Infinity", "inf", "-inf", "NA",
               "null", "NULL", "N/A", "1e", "1.5E", "2e+", "3E-", "1234567890123456",
               "-9223372036854775808", "-0", "-000", "1e309", "1e-309", "1234567890e300",
               "0.0001e-305", "1.8e308", "-1.8E308", "1e400", ".", "-", "+", "e5", "1.2.3", "1x",
               "0x10", "1_000", "--1", "1e5.0", "१२", "1e00000000000000005"]
# float text beyond the double range: pandas keeps such a column as text
OVERFLOW_CELLS = ["1e309", "9.999999999999999e308", "-123.456E+307", "1.8e308", "1234567890e300"]
# int-like text too wide for int64 (pandas types the column uint64 or object)
TOO_WIDE = ["9223372036854775808", "99999999999999999999", "-9223372036854775809"]


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_array(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- one cell ---------------------------------------------------------------------
E = [float(f"1e{i}") for i in range(309)]
_FLOAT_RE = re.compile(rb"([+-]?)(\d*)(?:(\.)(\d*))?(?:[eE]([+-]?)(\d+))?\Z")
_INT_RE = re.compile(rb"[+-]?\d+\Z")


def model_cell(text: bytes):
    """(kind, value) as csvp_cell gives them; value is None for DEFER."""
    if text == b"":
        return EMPTY, float("nan")
    i, n = 0, len(text)
    neg = text[:1] == b"-"
    if text[:1] in (b"-", b"+"):
        i = 1
    number, exponent, nd, i0, nonzero = 0.0, 0, 0, i, False
    while i < n and 48 <= text[i] <= 57:
        if nd < 17:
            number = number * 10.0 + float(text[i] - 48)
            nd += 1
        else:
            exponent += 1
        nonzero |= text[i] != 48
        i += 1
    int_digits, int_like = i - i0, True
    if i < n and text[i] == 46:
        int_like = False
        i += 1
        ndec = 0
        while nd < 17 and i < n and 48 <= text[i] <= 57:
            number = number * 10.0 + float(text[i] - 48)
            i, nd, ndec = i + 1, nd + 1, ndec + 1
        while i < n and 48 <= text[i] <= 57:
            i += 1
        exponent -= ndec
    if nd == 0:
        return DEFER, None
    if neg:
        number = -number
    if i < n and text[i] in (101, 69):
        int_like = False
        i += 1
        eneg = False
        if i < n and text[i] in (45, 43):
            eneg = text[i] == 45
            i += 1
        j = i
        while i < n and 48 <= text[i] <= 57:
            i += 1
        if i == j or i - j >= 17 or int(text[j:i]) >= 100000:
            return DEFER, None
        exponent += -int(text[j:i]) if eneg else int(text[j:i])
    if i != n:
        return DEFER, None
    if int_like:
        if int_digits > 15 or (neg and not nonzero):
            return DEFER, None
        return INT, number
    if exponent > 308 or exponent < -308:
        return DEFER, None
    number = number * E[exponent] if exponent > 0 else number / E[-exponent]
    if math.isinf(number):
        return DEFER, None
    return FLOAT, number


def expected_kind(text: bytes, value_is_inf: bool) -> int:
    """The kind from the text alone; value_is_inf: pandas read +-inf from it."""
    if text == b"":
        return EMPTY
    if _INT_RE.match(text):
        digits = text.lstrip(b"+-")
        if len(digits) > 15 or (text[:1] == b"-" and int(digits) == 0):
            return DEFER
        return INT
    m = _FLOAT_RE.match(text)
    if not m or not (m.group(2) or m.group(4)):
        return DEFER
    if m.group(6) is not None and len(m.group(6)) >= 17:
        return DEFER
    ip, fp = m.group(2) or b"", m.group(4) or b""
    exp = int(m.group(6) or 0) * (-1 if m.group(5) == b"-" else 1)
    taken_dec = max(0, min(len(fp), 17 - len(ip)))
    adjusted = max(0, len(ip) - 17) - taken_dec + exp
    if abs(exp) >= 100000 or not -308 <= adjusted <= 308 or value_is_inf:
        return DEFER
    return FLOAT


def pandas_column(texts) -> np.ndarray:
    """What pd.read_csv makes of a one-column file of these cells, as float64."""
    import pandas as pd

    buf = io.BytesIO(b"x\n" + b"\n".join(texts) + b"\n")
    return pd.read_csv(buf, skip_blank_lines=False)["x"].values.astype(np.float64)


def java_text(x: float) -> bytes:
    """A Java-like spelling (1.0E-4) of repr's digits: the writer's layouts."""
    r = repr(float(x))
    if "e" in r:
        mant, ex = r.split("e")
        if "." not in mant:
            mant += ".0"
        return f"{mant}E{int(ex)}".encode()
    if "." not in r:
        r += ".0"
    return r.encode()


@functools.lru_cache(maxsize=None)
def float_cells():
    """>= 200k float-grammar cells: repr and Java style of uniform values,
    ratios, values over 60 decades, raw bit patterns, 18 to 25 digit cells,
    exponents to +-308, -0.0, .5, 5. and friends."""
    rng = random.Random(20240611)
    out = [b"-0.0", b"0.0", b".5", b"5.", b"-.5", b"+5.", b"+0.5", b"0.1", b"1e0", b"1E5", b"1e-5",
           b"00012.5", b"000.000125", b"1.0000000000000000000000001", b"1e308", b"1e-308",
           b"1.7976931348623157e308", b"2.2250738585072014e-308", b"4.9e-308",
           b"12345678901234567890.0", b"0.00000000000000000000000012345678901234567890",
           b"123456789012345678901234567890e-20", b"9007199254740993.0", b"1.5e+10", b"1.5E-10"]
    for _ in range(60000):
        out.append(repr(rng.random()).encode())
    for _ in range(30000):
        out.append(java_text(rng.random() * 10 ** rng.randint(-8, 8)))
    for _ in range(30000):
        out.append(repr(rng.randint(0, 5000) / rng.randint(1, 5000)).encode())
    for _ in range(40000):
        v = rng.uniform(-1, 1) * 10.0 ** rng.randint(-30, 30)
        out.append(repr(v).encode() if rng.random() < 0.5 else java_text(v))
    while len(out) < 185000:  # raw bit patterns, finite, inside pandas' one-step range
        v = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if v == v and not math.isinf(v) and (v == 0.0 or 1e-290 < abs(v) < 1e290):
            out.append(repr(v).encode())
    for _ in range(15000):  # 18 to 25 digits around the point
        nd = rng.randint(18, 25)
        digits = "".join(rng.choice("0123456789") for _ in range(nd))
        cut = rng.randint(0, nd)
        txt = (digits[:cut] or "") + "." + digits[cut:]
        if rng.random() < 0.3:
            txt += f"e{rng.randint(-40, 40)}"
        out.append(txt.encode())
    for e in range(-308, 309):  # exponents to +-308 (some overflow: those defer)
        for m in ("1", "1.5", "9.999999999999999", "0.001", "123.456"):
            out.append(f"{m}e{e}".encode())
            out.append(f"-{m}E{e:+d}".encode())
    # a cell pandas reports a range error for turns the whole column into text
    # (OVERFLOW_CELLS are checked for their kind alone)
    return [t for t in out if abs(float(t)) <= 1.79e308]


@functools.lru_cache(maxsize=None)
def int_cells():
    rng = random.Random(77)
    out = [b"0", b"+0", b"7", b"-7", b"+12", b"007", b"999999999999999", b"-999999999999999",
           b"100000000000000", b"000000000000001"]
    for _ in range(3000):
        out.append(str(rng.randint(-10 ** rng.randint(1, 15) + 1, 10 ** rng.randint(1, 15) - 1)).encode())
    out += [str(rng.randint(10 ** 14, 10 ** 15 - 1)).encode() for _ in range(1000)]  # 15 digits
    return out


# ---- records and the guard ----------------------------------------------------------
def split_records(body: bytes):
    """(records, guard): records = [(begin, end)] of the body as csvin.hip's
    index gives them (plain quote parity; end excludes the terminator and its
    CR; begin is past the blank lines), guard = the first offset where plain
    parity is not pandas' quoting or a line of blanks starts, or -1."""
    n = len(body)
    ends, inq = [], False
    for p in range(n):
        ch = body[p]
        if ch == 34:
            inq = not inq
        elif ch == 10 and not inq:
            if p == 0 or body[p - 1] == 10:
                continue
            if body[p - 1] == 13 and (p == 1 or body[p - 2] == 10):
                continue
            ends.append(p)
    if inq:
        ends.append(n)
    elif n and body[n - 1] != 10 and not (body[n - 1] == 13 and (n < 2 or body[n - 2] == 10)):
        ends.append(n)
    records, guard, prev = [], -1, 0
    for e0 in ends:
        s = prev
        while s < n and (body[s] == 10 or (body[s] == 13 and body[s + 1:s + 2] == b"\n")):
            s += 1 if body[s] == 10 else 2
        e = e0 - 1 if e0 > s and body[e0 - 1] == 13 else e0
        prev = e0 + 1
        records.append((s, e))
        row = body[s:e]
        g = -1
        if row and row.strip(b" \t") == b"":
            g = s
        elif b'"' in row:
            g = _guard_walk(body, s, e)
        if g >= 0 and (guard < 0 or g < guard):
            guard = g
    return records, guard


def _guard_walk(buf, s, e):
    inq, k, open_at = False, s, -1
    while k < e:
        if buf[k] != 34:
            k += 1
            continue
        if not inq:
            if k != s and buf[k - 1] != 44:
                return k
            inq, open_at = True, k
        elif k + 1 < e and buf[k + 1] == 34:
            k += 1
        else:
            if k + 1 < e and buf[k + 1] not in (44, 13, 10):
                return k
            inq = False
        k += 1
    return open_at if inq else -1


def row_is_deferred(row: bytes, n_cols: int, sel) -> bool:
    """The parse kernel's rule for one record's bytes."""
    if b'"' in row or b"\0" in row or b"\r" in row:
        return True
    fields = row.split(b",")
    if len(fields) != n_cols:
        return True
    return any(model_cell(fields[j])[0] == DEFER for j in sel)


# ---- file builders -------------------------------------------------------------------
def quote_path(p: str) -> str:
    return '"' + p.replace('"', '""') + '"' if any(c in p for c in ',"\n\r') else p


def numeric_text(rng, style=None) -> str:
    """One cell of the kinds a features file holds: ratios, norms, counts, ages."""
    s = rng.random() if style is None else style
    if s < 0.35:
        return java_text(rng.randint(0, 4000) / rng.randint(1, 4000)).decode()
    if s < 0.6:
        return java_text(rng.random()).decode()
    if s < 0.75:
        return java_text(rng.randint(0, 4 * 10 ** 7) + rng.randint(0, 999) / 1000.0).decode()
    if s < 0.9:
        return java_text(rng.uniform(-1, 1) * 10.0 ** rng.randint(-12, 12)).decode()
    return str(rng.randint(0, 5000))


def table_text(n_rows, names, seed, path=lambda i: f"/data/set{i % 97:02d}/part-{i:08d}.bin"):
    """rows = list of lists of cell text; column 0 is the path.  Every numeric
    column holds at least one float cell (so pandas types none of them int64)."""
    rng = random.Random(seed)
    rows = []
    for i in range(n_rows):
        rows.append([path(i)] + [numeric_text(rng, 0.5 if i == 0 else None) for _ in names[1:]])
    return rows


def file_bytes(names, rows, eol=b"\n", last_eol=True) -> bytes:
    lines = [",".join(names).encode()] + [",".join([quote_path(r[0])] + r[1:]).encode("utf-8")
                                          for r in rows]
    data = eol.join(lines)
    return data + eol if last_eol else data


def pandas_x(data: bytes, columns) -> np.ndarray:
    import pandas as pd

    return pd.read_csv(io.BytesIO(data))[list(columns)].values.astype(np.float64)

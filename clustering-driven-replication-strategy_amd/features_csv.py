"""The features CSV read on the device, bit-identical to pandas.

Replaces the reference's ``src/main.py:75-81``::

    feature_file = pd.read_csv(input_csv_path)
    X = feature_file[CLUSTERING_FEATURES].values

for a caller that only needs X: ``read_features`` returns the same float64
bits and leaves the points resident in the context, so ``kmeans_csv`` runs
``kmeans`` on them without a second trip over the bus.  The records are found
and the cells parsed in libcdr.so (csrc/csvin.hip, csrc/csv_parse.h: pandas'
default float parser is not correctly rounded, and the kernel restates it step
by step).  What the device does not decide itself goes to pandas, never to a
guess:

* a deferred row (a quoted field, a field count other than the header's, a
  NUL or lone CR, a cell that is not plain float or short int text): pandas
  parses the header plus those rows' bytes;
* the whole file, through pandas and ``load_points``, when a quote stands
  where pandas' quoting differs from plain quote parity, when a line holds
  only blanks, when an int-like cell does not fit int64, or whenever pandas'
  view of the deferred rows does not line up with the device's.

pandas is imported on those paths only.
"""
from __future__ import annotations

import csv
import io
import mmap
import os

import numpy as np

from _cdr import Context, NanProbabilities, default_context

__all__ = ["CLUSTERING_FEATURES", "read_features", "kmeans_csv"]

# src/main.py:23-29
CLUSTERING_FEATURES = ["access_freq_norm", "age_norm", "write_ratio_norm", "locality_norm",
                       "concurrency_norm"]
MAX_DEVICE_COLUMNS = 16       # cdr_csv_read's d
DEFERRED_CAP = 1 << 20        # deferred rows taken back from the device in one read


def _header(data):
    """(names, body offset) of the header record, or None when the host
    tokeniser must look at it (a BOM, a quote where plain parity is not
    pandas' quoting, no header at all)."""
    n = len(data)
    pos = 0
    if data[:3] == b"\xef\xbb\xbf":
        return None
    while pos < n:  # pandas skips empty lines and lines of blanks
        end = data.find(b"\n", pos)
        line = data[pos:n if end < 0 else end]
        if line.strip(b" \t\r") != b"":
            break
        if end < 0:
            return None
        pos = end + 1
    if pos >= n:
        return None
    start = pos
    inq = False
    while True:  # the record's '\n' is the first one outside quotes
        end = data.find(b"\n", pos)
        stop = n if end < 0 else end
        if data[pos:stop].count(b'"') & 1:
            inq = not inq
        if end < 0 or not inq:
            break
        pos = end + 1
    if inq:
        return None
    rec = data[start:stop]
    body = stop + 1 if end >= 0 else n
    if rec.endswith(b"\r"):
        rec = rec[:-1]
    if b"\r" in rec or b"\0" in rec:
        return None
    if b'"' in rec:
        k, m = 0, len(rec)
        while k < m:  # the quote rule of the device guard
            if rec[k:k + 1] != b'"':
                k += 1
                continue
            if k and rec[k - 1:k] != b",":
                return None
            k += 1
            while True:
                q = rec.find(b'"', k)
                if q < 0:
                    return None
                if rec[q + 1:q + 2] == b'"':
                    k = q + 2
                    continue
                if q + 1 < m and rec[q + 1:q + 2] != b",":
                    return None
                k = q + 1
                break
    try:
        names = next(csv.reader(io.StringIO(rec.decode("utf-8"), newline="")))
    except (UnicodeDecodeError, StopIteration, csv.Error):
        return None
    return names, body


def _first_row_fields(data, body):
    """Field count of the first data line when it is plain (no quote), else -1."""
    n = len(data)
    pos = body
    while pos < n:
        end = data.find(b"\n", pos)
        line = data[pos:n if end < 0 else end]
        if line.strip(b" \t\r") != b"":
            return -1 if b'"' in line else line.count(b",") + 1
        if end < 0:
            break
        pos = end + 1
    return -1


def _whole_file(path, columns, ctx, info):
    """The reference's two lines, then ``load_points``: the host path."""
    import pandas as pd

    frame = pd.read_csv(path)[list(columns)]
    for name, dt in zip(frame.columns, frame.dtypes):
        if dt.kind not in "iuf":
            raise ValueError(f"column {name!r} is not numeric (pandas reads it as {dt})")
    X = np.ascontiguousarray(frame.values.astype(np.float64)).reshape(len(frame), len(columns))
    info.update(rows=int(X.shape[0]), deferred_rows=0, whole_file_fallback=True, resident=False)
    try:
        ctx.load_points(X)
        info["resident"] = True
    except NanProbabilities:  # X is what pandas read; kmeans on it raises as the reference does
        pass
    return X


def _patch_rows(data, header_end, deferred, names, columns, kinds):
    """pandas' values (m, d) of the deferred rows, or None when its view of
    them does not line up with the device's (the whole file is read then)."""
    import pandas as pd

    parts = [bytes(data[:header_end])]
    if not parts[0].endswith(b"\n"):
        parts.append(b"\n")
    # pandas infers an index from a first data row with more fields than the
    # header; a plain first row (dropped below) keeps the header's meaning
    parts.append(b",".join([b"0"] * len(names)) + b"\n")
    for _, b0, b1 in deferred:
        parts.append(bytes(data[int(b0):int(b1)]))
        parts.append(b"\n")
    # pandas types a column int64 only when every cell is int-like; the device
    # has seen all the other rows
    dtype = {c: (np.int64 if kinds[j, 1] == 0 and kinds[j, 2] == 0 else np.float64)
             for j, c in enumerate(columns)}
    try:
        # (no usecols: with it pandas lets a row with too many fields pass)
        frame = pd.read_csv(io.BytesIO(b"".join(parts)), dtype=dtype)
    except Exception:  # an int that does not fit, text in the column, a ragged row, ...
        return None
    if len(frame) != len(deferred) + 1:  # (a lone CR ends a record for pandas)
        return None
    if any(frame[c].dtype != np.dtype(t) for c, t in dtype.items()):  # (uint64 for a wide int)
        return None
    return np.ascontiguousarray(frame[list(columns)].values[1:].astype(np.float64))


def read_features(path, columns=CLUSTERING_FEATURES, ctx: Context | None = None,
                  info: dict | None = None) -> np.ndarray:
    """``pd.read_csv(path)[columns].values.astype(np.float64)``, bit for bit
    (NaN cells included), with the points left resident in ``ctx``.

    ``info`` (a dict, filled in place) receives ``rows``, ``deferred_rows``,
    ``whole_file_fallback``, ``resident`` (False only when a cell is not finite:
    ``load_points`` refuses such points too), ``guard`` and the kernel times
    ``upload_ms``, ``index_ms``, ``parse_ms``, ``finish_ms``."""
    ctx = ctx if ctx is not None else default_context()
    info = info if info is not None else {}
    info.clear()
    columns = list(columns)
    size = os.path.getsize(path)
    if size == 0:
        return _whole_file(path, columns, ctx, info)  # pandas' EmptyDataError
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as data:
        head = _header(data)
        if head is None:
            return _whole_file(path, columns, ctx, info)
        names, body = head
        plain = (len(set(names)) == len(names) and all(names) and len(set(columns)) == len(columns)
                 and 1 <= len(columns) <= MAX_DEVICE_COLUMNS and len(names) <= 32767
                 and _first_row_fields(data, body) in (-1, len(names)) and body < size)
        if not plain:
            # names pandas would mangle, a first row that makes pandas infer an
            # index, repeated or too many columns, no data rows
            return _whole_file(path, columns, ctx, info)
        if any(c not in names for c in columns):
            import pandas as pd

            pd.DataFrame(columns=names)[columns]  # pandas' own KeyError for the indexing
        sel = [names.index(c) for c in columns]
        res = ctx.csv_read(data, body, len(names), sel, DEFERRED_CAP)
        t = ctx.csv_read_timing()
        info.update(rows=res["rows"], deferred_rows=res["deferred_rows"], guard=res["guard"],
                    whole_file_fallback=False, upload_ms=float(t[0]), index_ms=float(t[1]),
                    parse_ms=float(t[2]), finish_ms=0.0)
        values = np.zeros((0, len(columns)))
        if res["guard"] >= 0 or res["deferred_rows"] > len(res["deferred"]):
            values = None
        elif res["deferred_rows"]:
            values = _patch_rows(data, body, res["deferred"], names, columns, res["col_kinds"])
        rows = res["deferred"][:, 0] if values is not None else None
    if values is None:
        return _whole_file(path, columns, ctx, info)
    info["resident"] = True
    try:
        X = ctx.csv_read_finish(rows, values)
    except NanProbabilities as e:  # an empty cell: X is complete, the points are not usable
        X = e.X
        info["resident"] = False
    info["finish_ms"] = float(ctx.csv_read_timing()[3])
    return X


def kmeans_csv(path, k, columns=CLUSTERING_FEATURES, tol=1e-4, random_state=None, *,
               max_iter=None, context: Context | None = None):
    """``kmeans(pd.read_csv(path)[columns].values, k, number_of_files=n, ...)``
    as main.py:75-91 calls it, with X read on the device and never uploaded
    again.  ``max_iter=None`` keeps the reference's rule (max(100, n / 100): a
    TypeError above 10 000 rows, kmeans_plusplus.py)."""
    from kmeans_plusplus import _kmeans_loaded

    ctx = context if context is not None else default_context()
    info: dict = {}
    X = read_features(path, columns, ctx=ctx, info=info)
    if not info.get("resident"):
        ctx.load_points(X)  # raises what kmeans(X, ...) raises for such an X
    return _kmeans_loaded(ctx, X, k, X.shape[0], tol, random_state, max_iter)

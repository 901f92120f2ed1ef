"""Shared inputs of the replication-plan tests, and a host-backed stand-in for
the context so that the CPU suite can run write_plan_csv's chunking and splice.

The expected bytes always come from ``write_plan_csv_host`` (the definition) or
from an independent restatement of it, never from the code under test."""
import numpy as np

import csv_read_cases as rc

FACTORS = {"Hot": 3, "Shared": 2, "Moderate": 1, "Archival": 4}
CATS4 = {"C0": "Moderate", "C1": "Hot", "C2": "Archival", "C3": "Shared"}
MAX_FIELD = 65535      # plan.hip kPlanMaxField
BLOCK = 256            # rows per workgroup of plan.hip's kernels (kPlanBlock)
SCAN_TOP = 256 * 256   # rows up to which csv_scan_top's threads take one workgroup sum each


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def put(path, data):
    with open(path, "wb") as fh:
        fh.write(data)
    return str(path)


def plain_file(n, seed=1, path=lambda i: f"/data/set{i % 97:02d}/part-{i:08d}.bin", **kw):
    """An 11-column features file of n plain rows."""
    return rc.file_bytes(rc.HEADER11, rc.table_text(n, rc.HEADER11, seed=seed, path=path), **kw)


def labels_for(n, k, seed=0):
    lab = np.random.default_rng(seed).integers(0, k, size=n)
    if n:
        lab[0], lab[-1] = k - 1, 0
    return lab.astype(np.int64)


def tails_of(cats, facs):
    return [f",{c},{f}\n".encode() for c, f in zip(cats, facs)]


class FakeCtx:
    """plan_format as the device gives it, computed on the host from
    csv_read_cases.split_records; rows in `defer` are deferred on top of the
    rows the device defers by its own rule."""

    def __init__(self, defer=(), resident=None):
        self.defer = set(defer)
        self.resident = resident
        self.calls = []

    def labels(self):
        return np.asarray(self.resident, dtype=np.int64)

    def info(self):
        return {"n": len(self.resident)}

    def plan_bound(self, n_rows, field_bytes):
        return field_bytes + n_rows * 74

    def plan_timing(self):
        return np.zeros(5)

    def plan_format(self, data, body_off, n_cols, path_col, labels, k, tails, row_begin=0,
                    row_count=None, out=None, deferred_cap=1 << 20):
        data = bytes(data)
        body = data[body_off:]
        records, guard = rc.split_records(body)
        labels = self.labels() if labels is None else labels
        if len(labels) != len(records):
            raise ValueError(f"plan: {len(labels)} labels, the file has {len(records)} rows")
        hi = len(records) if row_count is None else min(len(records), row_begin + row_count)
        self.calls.append((row_begin, hi - row_begin))
        parts, deferred, off, prev = [], [], 0, 0
        for r, (s, e) in enumerate(records):
            row = body[s:e]
            end = e + 1 if body[e:e + 1] == b"\r" else e  # the terminator's index
            begin, prev = prev, end + 1
            if not row_begin <= r < hi:
                continue
            fields = row.split(b",")
            if (r in self.defer or b'"' in row or b"\0" in row or b"\r" in row
                    or len(fields) != n_cols or len(fields[path_col]) > MAX_FIELD):
                deferred.append((r, off, body_off + begin, body_off + end))
                continue
            parts.append(fields[path_col] + b"," + str(int(labels[r])).encode() + tails[int(labels[r])])
            off += len(parts[-1])
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        return {"rows": len(records), "text": text, "deferred_rows": len(deferred),
                "deferred": np.array(deferred[:deferred_cap], dtype=np.int64).reshape(-1, 4),
                "guard": -1 if guard < 0 else guard + body_off}

    def plan_size_sums(self, sizes, k, labels=None):
        labels = self.labels() if labels is None else labels
        sizes = np.ones(len(labels), dtype=np.int64) if sizes is None else sizes
        out = [0] * k
        for s, l in zip(np.asarray(sizes).tolist(), np.asarray(labels).tolist()):
            if s < 0 or not 0 <= l < k:
                raise ValueError("size or label")
            out[l] += s
        return out

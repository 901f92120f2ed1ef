"""Two clusterings of the same files compared: contingency table, adjusted
Rand index, cluster matching.

An extension with no counterpart in the reference, which forms the cluster
column once and drops it (src/main.py:92).  k-means is seeded anew for every
access log, so today's cluster numbers mean something else than yesterday's;
everything that relates two labelings a and b of the same n rows starts from
one table::

    T[i][j] = number of rows r with a[r] == i and b[r] == j

and, with one int64 size per row, the bytes of each cell.  ``contingency_host``
is the definition (NumPy, no GPU).  ``contingency`` gives the same integers
from libcdr.so (csrc/agree.hip) without a label leaving the device: the `a`
side defaults to the labels of the last assignment resident in the context,
the `b` side to the labels ``keep()`` copied on the device after an earlier
run.  The adds are integers, so the two agree with ``==``.

The table feeds ``adjusted_rand`` (is a k stable across seeds:
``cluster_quality.stability``), ``match_clusters`` (which new cluster is which
old one) and ``replication_plan.transition`` (what a new plan changes).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from _cdr import Context, default_context

__all__ = ["contingency", "contingency_host", "adjusted_rand", "match_clusters", "keep"]

MAX_K = 1024  # cdr_agree_table's ka and kb


def _labels(labels, k, name):
    labels = np.asarray(labels).astype(np.int64, copy=False).ravel()
    if labels.size and (labels.min() < 0 or labels.max() >= k):
        raise ValueError(f"{name}: a label outside [0, {k})")
    return labels


def contingency_host(labels_a, labels_b, ka, kb, sizes=None):
    """The definition.  counts: int64 (ka, kb) by ``np.add.at`` of ones.  With
    `sizes` (int64 >= 0, one per row) returns ``(counts, bytes)``: bytes an
    object array (ka, kb) of Python ints, ``lo + (hi << 32)`` of two uint64
    ``np.add.at`` sums of the sizes' low 32 and high 31 bits (neither overflows
    below 2^31 rows, their combination can pass uint64)."""
    ka, kb = int(ka), int(kb)
    if ka < 1 or kb < 1:
        raise ValueError("ka and kb must be at least 1")
    a = _labels(labels_a, ka, "labels_a")
    b = _labels(labels_b, kb, "labels_b")
    if a.size != b.size:
        raise ValueError(f"{a.size} labels against {b.size}")
    counts = np.zeros((ka, kb), dtype=np.int64)
    np.add.at(counts, (a, b), 1)
    if sizes is None:
        return counts
    s = np.asarray(sizes).astype(np.int64, copy=False).ravel()
    if s.size != a.size:
        raise ValueError(f"{s.size} sizes for {a.size} rows")
    if s.size and s.min() < 0:
        raise ValueError("negative size")
    u = s.astype(np.uint64)
    lo = np.zeros((ka, kb), dtype=np.uint64)
    hi = np.zeros((ka, kb), dtype=np.uint64)
    np.add.at(lo, (a, b), u & np.uint64(0xFFFFFFFF))
    np.add.at(hi, (a, b), u >> np.uint64(32))
    return counts, lo.astype(object) + hi.astype(object) * (1 << 32)


def contingency(labels_a=None, labels_b=None, *, ka, kb, sizes=None,
                context: Context | None = None):
    """``contingency_host`` on the device (one cdr_agree_table call).
    ``labels_a=None``: the labels of the last assignment resident in `context`
    (ka >= their k); ``labels_b=None``: the labels ``keep()`` copied (kb >=
    their k).  1 <= ka, kb <= 1024 (NotImplementedError beyond); ValueError for
    a label out of range, a negative size or a row count that does not match;
    RuntimeError for a None side with nothing resident or kept."""
    ctx = context if context is not None else default_context()
    return ctx.agree_table(ka, kb, labels_a, labels_b, sizes)


def keep(context: Context | None = None) -> None:
    """Keeps the resident labels on the device (cdr_agree_keep) as the `b` side
    of later ``contingency(labels_b=None)`` calls; they survive later k-means
    runs and ``load_points``."""
    ctx = context if context is not None else default_context()
    ctx.agree_keep()


def _pairs(v) -> int:
    """sum of C(v, 2), in int64: every sum here is at most C(2^31, 2) < 2^61."""
    v = np.asarray(v, dtype=np.int64)
    return int(np.sum(v * (v - 1) // 2, dtype=np.int64))


def adjusted_rand(table) -> float:
    """The adjusted Rand index of a contingency table of n < 2^31 rows.  With
    s = sum C(n_ij, 2), a = sum C(row_i, 2), b = sum C(col_j, 2), N = C(n, 2):
    ``2 (s N - a b) / ((a + b) N - 2 a b)``, the products in Python ints and the
    quotient as a Fraction rounded to float once; 1.0 when the denominator is 0
    (scikit-learn's fn == fp == 0: one cluster on both sides, all singletons,
    fewer than 2 rows)."""
    t = np.asarray(table)
    if t.ndim != 2:
        raise ValueError("the table must be 2-D")
    t = t.astype(np.int64)
    if t.size and t.min() < 0:
        raise ValueError("negative count")
    n = int(t.sum(dtype=np.int64))
    if n >= 1 << 31:
        raise ValueError("the table holds 2^31 rows or more")
    s = _pairs(t)
    a = _pairs(t.sum(axis=1, dtype=np.int64))
    b = _pairs(t.sum(axis=0, dtype=np.int64))
    big = n * (n - 1) // 2
    den = (a + b) * big - 2 * a * b
    if den == 0:
        return 1.0
    return float(Fraction(2 * (s * big - a * b), den))


def match_clusters(table) -> np.ndarray:
    """For every b-cluster (column) the a-cluster (row) it is matched to, int64
    (kb,), in the one-to-one assignment that maximises the matched row count
    (``scipy.optimize.linear_sum_assignment(table, maximize=True)``); -1 for the
    b-clusters a table with more columns than rows leaves unmatched."""
    from scipy.optimize import linear_sum_assignment

    t = np.asarray(table)
    if t.ndim != 2:
        raise ValueError("the table must be 2-D")
    rows, cols = linear_sum_assignment(t.astype(np.int64), maximize=True)
    out = np.full(t.shape[1], -1, dtype=np.int64)
    out[cols] = rows
    return out

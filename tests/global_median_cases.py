"""Point sets for the global-median tests (TEST INFRASTRUCTURE ONLY).

``case(name)`` returns ``(X, expected)``: the float64 table a test loads and
``np.median(X, axis=0)`` of it (NaN for n = 0).  tests/test_global_median_cases.py
checks every expected value on the CPU against the sorted-value contract at the
top of csrc/medians.hip; tests/test_gpu_global_medians.py loads each table and
asks the device for the same bits.

Modes: ``f32x`` tables hold fp32-exact values on a grid coarse enough for F32X
storage; ``f64`` tables hold doubles that no float32 holds (F64 storage).

Families
  rows-N-mode      N x 3, every value in [1, 2): a counted padding row (a zero)
                   would move the median
  grid-mode        70 001 x 5 (the grid-stride test)
  feat-D-mode      1037 x D, signed values
  part-N-mode      N = 600 / 601 rows, planted columns (``part_notes``): what
                   the two middle values are
  degen-N-mode     N = 10 000 / 10 001 rows x 8 (``DEGEN_NOTES``)
  minmax           12 000 x 5 min-max doubles (the scoring test)
"""
from __future__ import annotations

import functools

import numpy as np

import median_cases as mc

# constants of csrc/medians.hip the cases are sized by
GM_ROWS = 512     # kGmRows: rows per wave turn of gm_hist32 / gm_hist64
GM_WAVES = 4      # kGmThreads / 64: waves per workgroup (one turn of a workgroup
                  # at one quad / one feature per chunk = GM_WAVES * GM_ROWS rows)
GM_FEAT = 16      # kGmFeat: features per histogram workgroup
ROW_PAD = 8192    # kSeedBlock: rows are padded to a multiple of it with zeros

MODES = ("f32x", "f64")
ROW_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 16385,
         GM_ROWS - 1, GM_ROWS, GM_ROWS + 1,
         GM_WAVES * GM_ROWS - 1, GM_WAVES * GM_ROWS, GM_WAVES * GM_ROWS + 1)
GRID_N = 70_001
FEAT_D = (1, 2, 3, 4, 5, 16, 17, 64, 65, 128)
FEAT_N = 1037
PART_N = (600, 601)
DEGEN_N = (10_000, 10_001)
DEGEN_NOTES = ("constant", "two values 1:1", "two values 1:(n-1)", "half one value, rest random",
               "random", "constant among random quad neighbours", "random", "random")


def _unit(rng, shape, mode, lo=1.0):
    """Values in [lo, lo + 1): on the 2^-20 grid (f32x) or full doubles."""
    if mode == "f32x":
        return lo + rng.integers(0, 1 << 20, shape) / float(1 << 20)
    return lo + rng.random(shape)


def _signed(rng, shape, mode):
    if mode == "f32x":
        return rng.integers(-(1 << 19), 1 << 19, shape) / float(1 << 16)
    return rng.normal(0.0, 3.0, shape)


def _nxt(v, mode):
    if mode == "f32x":
        return float(np.nextafter(np.float32(v), np.float32(np.inf)))
    return float(np.nextafter(v, np.inf))


def part_notes(mode):
    """(note, anchor, lo, hi) of the planted columns: lo <= hi are the values
    around the middle."""
    rng = np.random.default_rng(77)
    out = [("equal", 0.0, 0.125, 0.125),
           ("neighbours", 0.0, 0.5, _nxt(0.5, mode)),
           ("opposite sign", 0.0, -0.25, 0.25)]
    if mode == "f64":
        out.append(("signed zeros", 0.0, -0.0, 0.0))
    for p in range(4 if mode == "f32x" else 8):
        j, lo, hi = mc.byte_pair(p, mode, rng)
        out.append(("byte %d" % p, 4.0 * j, lo, hi))
    return out


def _part(n, mode):
    """Even n: the two middle values are (lo, hi).  Odd n: the middle three are
    (lo, hi, hi), so the one middle rank sits on hi with lo right below it."""
    rng = np.random.default_rng(100 + n)
    cols = []
    for note, anchor, lo, hi in part_notes(mode):
        mid = [lo, hi] if n % 2 == 0 else [lo, hi, hi]
        cols.append(rng.permutation(mc.column(n, anchor, mid, mode)))
    return np.stack(cols, axis=1)


def _degen(n, mode):
    rng = np.random.default_rng(200 + n)
    X = _unit(rng, (n, 8), mode, lo=0.0)
    X[:, 0] = 0.375
    X[:, 1] = np.where(rng.permutation(n) < n // 2, 0.25, 0.75)
    X[:, 2] = 0.25
    X[int(rng.integers(n)), 2] = 0.75
    half = rng.permutation(n) < n // 2 + 1
    X[half, 3] = 0.5
    X[:, 5] = 0.625
    if mode == "f64":
        X[:, [4, 6, 7]] += np.pi * 2.0 ** -30
    return X


def minmax(n, d, seed):
    """Min-max normalised doubles (skewed, full mantissas)."""
    rng = np.random.default_rng(seed)
    raw = rng.gamma(2.0, 3.0, (n, d)) * (0.2 + rng.random(d)) + rng.normal(0, 1, (n, d))
    return (raw - raw.min(axis=0)) / (raw.max(axis=0) - raw.min(axis=0))


def _build(name):
    kind, *rest = name.split("-")
    mode = rest[-1] if rest else "f64"
    if kind == "rows":
        n = int(rest[0])
        return _unit(np.random.default_rng(n), (n, 3), mode)
    if kind == "grid":
        return _signed(np.random.default_rng(9), (GRID_N, 5), mode)
    if kind == "feat":
        d = int(rest[0])
        return _signed(np.random.default_rng(300 + d), (FEAT_N, d), mode)
    if kind == "part":
        return _part(int(rest[0]), mode)
    if kind == "degen":
        return _degen(int(rest[0]), mode)
    if kind == "minmax":
        return minmax(12_000, 5, 46)
    raise KeyError(name)


CASES = tuple(
    ["rows-%d-%s" % (n, m) for n in ROW_N for m in MODES]
    + ["grid-%s" % m for m in MODES]
    + ["feat-%d-%s" % (d, m) for d in FEAT_D for m in MODES]
    + ["part-%d-%s" % (n, m) for n in PART_N for m in MODES]
    + ["degen-%d-%s" % (n, m) for n in DEGEN_N for m in MODES]
    + ["minmax"])


def np_medians(X):
    """np.median of every column; NaN for an empty table (no warning)."""
    if X.shape[0] == 0:
        return np.full(X.shape[1], np.nan)
    return np.median(X, axis=0)


def sort_medians(X):
    """The contract at the top of csrc/medians.hip, from the sorted values."""
    n = X.shape[0]
    if n == 0:
        return np.full(X.shape[1], np.nan)
    s = np.sort(X, axis=0)
    if n & 1:
        return (0.0 + s[n // 2]) / 1.0
    return ((0.0 + s[(n - 1) // 2]) + s[n // 2]) / 2.0


def is_f32x(X):
    return bool(np.array_equal(X.astype(np.float32).astype(np.float64), X))


@functools.lru_cache(maxsize=8)
def case(name):
    """(X, expected) of a named case; both read-only."""
    X = np.ascontiguousarray(_build(name), dtype=np.float64)
    exp = np_medians(X)
    X.setflags(write=False)
    exp.setflags(write=False)
    return X, exp


# ---- shards ----------------------------------------------------------------
SHARD_SPLITS = {
    "three": (5912, 319, 5),        # very uneven
    "parity": (41, 61),             # odd + odd = even
    "empty": (700, 0, 301),         # a rank without rows
}


def shard_case(name, mode):
    """(list of shard tables, expected medians of their union), d = 3."""
    sizes = SHARD_SPLITS[name]
    n = sum(sizes)
    X = _signed(np.random.default_rng(400 + n), (n, 3), mode)
    cut = np.concatenate([[0], np.cumsum(sizes)])
    return [X[cut[i]:cut[i + 1]] for i in range(len(sizes))], np_medians(X)


def split_middle_case(mode):
    """Two shards of 500 rows: shard 0 holds the 500 smallest values of every
    column and shard 1 the 500 largest, so the two middle values (ranks 499
    and 500) lie on different shards."""
    X = np.sort(_signed(np.random.default_rng(500), (1000, 3), mode), axis=0)
    rng = np.random.default_rng(501)
    return [rng.permutation(X[:500]), rng.permutation(X[500:])], np_medians(X)

"""Inputs of the features-CSV tests and their expected text.

The expected text always comes from the host code of compute_features
(java_double_legacy, str(int(v)), csv.writer as write_spark_csv uses it), never
from the code under test.  Everything is computed once per process."""
import csv
import functools
import io
import math
import random
import struct

import numpy as np

# both pinned lists of tests/test_host_logic.py (JDK bug 4511638 and the layouts)
PINNED = [2.82879384806159e17, 1.387364135037754e18, 1.45800632428665e17, 5.684341886080802e-14,
          8.41e21, 1.9400994884341945e25, 2e23, 2.0 ** 60, 2.0 ** 62, 2.0 ** 63, 2.0 ** 53,
          5e-324, 1.7976931348623157e308]
PINNED = PINNED + [-v for v in PINNED]
LAYOUTS = [0.0, -0.0, 1.0, 0.5, 100.0, 1e7, 1e-3, 9.99e-4, 1e-5, 9999999.5, 0.1 + 0.2, -2.5e-7,
           float("nan"), float("inf"), float("-inf"), 1.0 / 3, 123456789.0, 1234567.0,
           12277768.082999945]
LO, HI = 2.0 ** -128, 2.0 ** 128  # the device range: LO <= |x| < HI
EDGES = [1e-3, 9.99e-4, 1e7, 9999999.5, 0.0, -0.0, float("nan"), float("inf"), float("-inf"),
         LO, math.nextafter(HI, 0.0), -LO, -math.nextafter(HI, 0.0)]
# the designed deferrals: the neighbours of the range, a subnormal, the largest subnormal
OUTSIDE = [math.nextafter(LO, 0.0), HI, 5e-324, 2.2250738585072009e-308]
# d x 10^e in E-notation: about half of these doubles lie just below the decimal,
# where the digit loop ends on a 9 and the rounding carries through it (random
# values do not get there: a digit after the first stops the loop before a 9
# can be rounded up, except right after the forced second digit of E-notation)
ROUND = [float(f"{d}e{e}") for d in range(1, 10) for e in list(range(-37, -4)) + list(range(23, 38))]
# four mantissas of every binade of the device range (the widest multi-word
# operands are at the small end, csv_digits.h)
BINADES = [struct.unpack("<d", struct.pack("<Q", ((e + 1023) << 52) | m))[0]
           for e in range(-128, 128) for m in (0, 1, 1 << 51, (1 << 52) - 1)]
LONGS = [0.0, 1.0, -7.0, 2.7, -2.7, 2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 63 - 1024]
LONGS_DEFERRED = [2.0 ** 63, float("nan")]

RANDOM_SEED, FEATURE_SEED = 7, 11


def in_device_range(x: float) -> bool:
    """What the device formats itself: NaN, the infinities, zeros, and every
    finite double with 2^-128 <= |x| < 2^128."""
    return x != x or math.isinf(x) or x == 0.0 or LO <= abs(x) < HI


def random_values(n=60000, seed=RANDOM_SEED):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        v = rng.uniform(-1, 1) * 10 ** rng.randint(-30, 30)
        if rng.random() < 0.2:
            v = float(rng.getrandbits(rng.randint(1, 63)))
        out.append(v)
    return out


def feature_table(rows, seed=FEATURE_SEED):
    """A feature-like (rows, 10) table in OUT_COLUMNS[1:] order: counts, ages
    with a millisecond fraction, ratios of counts, min-max norms."""
    rng = np.random.default_rng(seed)
    freq = rng.integers(1, 5000, rows)
    writes = (freq * rng.random(rows)).astype(np.int64)
    age = rng.integers(0, 4 * 10 ** 7, rows) + rng.integers(0, 1000, rows) / 1000.0
    local = (freq * rng.random(rows)).astype(np.int64)
    conc = rng.integers(1, 64, rows)
    t = np.zeros((rows, 10))
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4] = freq, age, writes / freq, local / freq, conc
    for j in range(5):
        lo, hi = t[:, j].min(), t[:, j].max()
        t[:, 5 + j] = (t[:, j] - lo) / (hi - lo) if hi > lo else 0.0
    return t


def feature_paths(rows):
    return [f"/data/set{i % 97:02d}/part-{i:08d}.parquet" for i in range(rows)]


def feature_values(n=20000, seed=FEATURE_SEED):
    """n feature-like values: the table's counts, ages, ratios and norms."""
    t = feature_table(n // 4, seed)
    return np.stack([t[:, 0], t[:, 1], t[:, 2], t[:, 6]], axis=1).ravel().tolist()


@functools.lru_cache(maxsize=None)
def double_cases():
    """(values, expected text or None when deferred) of the double tests."""
    from compute_features import java_double_legacy

    vals = PINNED + LAYOUTS + EDGES + OUTSIDE + ROUND + BINADES + random_values() + feature_values()
    exp = [java_double_legacy(v) if in_device_range(v) else None for v in vals]
    return vals, exp


def host_rows(paths, table, long_cols=()):
    """The rows' text as write_spark_csv formats them (general column count)."""
    from compute_features import java_double_legacy

    buf = io.StringIO(newline="")
    w = csv.writer(buf, lineterminator="\n")
    rows = []
    for pth, vals in zip(paths, table):
        w.writerow([pth] + [str(int(v)) if j in long_cols else java_double_legacy(v)
                            for j, v in enumerate(vals)])
        rows.append(buf.getvalue().encode("utf-8"))
        buf.seek(0)
        buf.truncate()
    return rows


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]

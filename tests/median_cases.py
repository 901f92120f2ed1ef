"""Labelled point sets for the median tests (TEST INFRASTRUCTURE ONLY).

``labelled_points(sizes, d, mode, seed)`` builds points whose nearest centroid
is known by construction, so a test can ask for exact cluster sizes (1, 2, a
loop boundary of a kernel, ...) and still get them from a real Lloyd step:

* cluster j has exactly ``sizes[j]`` rows (0 allowed), shuffled over the rows
  so that every cluster spans the counting-sort blocks of medians.hip;
* row i is ``anchor[labels[i]] + e_i`` with ``anchor[j] = 4 j`` in every
  feature and ``|e| <= 63/64`` per feature: the own anchor is nearer than any
  other by a factor > 3 in every feature, so ``C = anchors`` assigns the
  designed labels with no ties (tests/test_median_cases.py checks it with the
  oracle);
* ``mode="f32x"`` keeps e on the 2^-6 grid (|x| 2^6 < 2^30 up to k = 8192, so
  the points are stored as F32X); ``mode="f64"`` adds a multiple of
  pi 2^-20 below 2^-8 to every value, which no float32 holds (F64 storage).

``plants`` replaces whole (cluster, feature) columns by values built with
``column`` below: chosen middle values, padded below and above inside the
cluster's ball.  The two middle ranks of such a column are then known, and
with them the radix pass at which the two selections part.

``CASES`` names every point set the GPU tests use (tests/
test_gpu_medians_shapes.py); the CPU test walks all of them.
"""
from __future__ import annotations

import functools

import numpy as np

MODE_F32X, MODE_F64 = 1, 2
SPACING = 4.0
EMAX = 63.0 / 64.0

# constants of csrc/medians.hip the cases are sized by; the GPU tests assert
# the property each case is there for from these, next to the case
MG_BLOCK = 4096   # kMgBlock: points per counting-sort block
MG_RANGE = 64     # kMgRange: blocks per column-scan range
MG_MAXK = 8192    # kMgMaxK
MG_WAVES = 16     # waves of an mg_hist workgroup
MG_U = 8          # kU: rows in flight per lane


def anchors(k: int, d: int) -> np.ndarray:
    return np.repeat(SPACING * np.arange(k, dtype=np.float64)[:, None], d, axis=1)


def hist_rows(d: int) -> int:
    """R = 16 (64 / D2): rows one mg_hist workgroup takes per step at this d
    (D2 the next power of two >= min(d, 64)); 8 R rows per unrolled turn."""
    D2 = 1
    while D2 < min(d, 64):
        D2 <<= 1
    return MG_WAVES * (64 // D2)


def column(size: int, anchor: float, middle, mode: str) -> np.ndarray:
    """``size`` values inside the ball of ``anchor`` whose sorted middle is
    ``middle`` (a sequence: its values sit symmetrically around the two middle
    ranks, so a run of ties passes through both).  The other values lie
    strictly below min(middle) and strictly above max(middle)."""
    mid = np.asarray(middle, dtype=np.float64)
    assert 1 <= mid.size <= size and (size - mid.size) % 2 == 0, (size, mid.size)
    assert np.all(np.abs(mid - anchor) < 0.74), (anchor, mid)
    side = (size - mid.size) // 2
    step = np.arange(side) % 16 / 64.0
    lows = anchor - EMAX + step                 # [a - 63/64, a - 48/64]
    highs = anchor + EMAX - step                # [a + 48/64, a + 63/64]
    if mode == "f64":
        lows = lows + np.pi * 2.0 ** -20
        highs = highs - np.pi * 2.0 ** -20
    return np.concatenate([lows, mid, highs])


def byte_pair(p: int, mode: str, rng) -> tuple[int, float, float]:
    """(cluster, lo, hi): two values of that cluster's ball whose
    order-preserving keys agree in the bytes above byte p (0 = the most
    significant, the first radix pass) and differ in byte p; the bytes below
    are random.  Keys are 4 bytes in F32X and 8 in F64."""
    if mode == "f32x":
        if p == 0:          # 0x3E.. against 0x3F..: binades [0.125, 0.5) and [0.5, 2)
            return 0, 0.25, 0.5
        sh = 8 * (3 - p)
        base = np.uint32(0x40800000)  # 4.0
        lo = base | np.uint32(1 << sh) | np.uint32(rng.integers(0, 1 << sh))
        hi = base | np.uint32(2 << sh) | np.uint32(rng.integers(0, 1 << sh))
        v = np.array([lo, hi], dtype=np.uint32).view(np.float32).astype(np.float64)
        return 1, float(v[0]), float(v[1])
    if p == 0:              # 0x3E.. against 0x3F..: below and above 2^-15
        return 0, 2.0 ** -20, 0.5
    sh = 8 * (7 - p)
    base = 0x4010000000000000     # 4.0
    lo = base | (1 << sh) | int(rng.integers(0, 1 << sh))
    hi = base | (2 << sh) | int(rng.integers(0, 1 << sh))
    v = np.array([lo, hi], dtype=np.uint64).view(np.float64)
    return 1, float(v[0]), float(v[1])


def labelled_points(sizes, d: int, mode: str, seed: int, plants=()):
    """(X (n, d) float64, C (k, d) = the anchors, labels (n,) int64)."""
    assert mode in ("f32x", "f64")
    sizes = np.asarray(sizes, dtype=np.int64)
    k = sizes.size
    rng = np.random.default_rng(seed)
    lab = np.repeat(np.arange(k, dtype=np.int64), sizes)
    n = lab.size
    C = anchors(k, d)
    e = rng.integers(-62, 63, (n, d)) / 64.0           # the 2^-6 grid, |e| <= 62/64
    if mode == "f64":
        e = e + np.pi * 2.0 ** -20 * rng.integers(1, 1 << 10, (n, d))   # + (0, 2^-8)
    X = C[lab] + e
    for j, f, vals in plants:
        vals = np.asarray(vals, dtype=np.float64)
        assert vals.size == sizes[j], (j, f, vals.size, sizes[j])
        assert np.all(np.abs(vals - C[j, f]) <= EMAX), (j, f)
        X[lab == j, f] = rng.permutation(vals)
    perm = rng.permutation(n)
    X, lab = np.ascontiguousarray(X[perm]), lab[perm]
    if mode == "f32x":
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    else:
        assert n == 0 or not np.array_equal(X.astype(np.float32).astype(np.float64), X)
    return X, C, lab


def ref_medians(X: np.ndarray, lab: np.ndarray, k: int) -> np.ndarray:
    """np.median of every cluster's columns; NaN rows for empty clusters."""
    out = np.full((k, X.shape[1]), np.nan)
    order = np.argsort(lab, kind="stable")
    bounds = np.searchsorted(lab[order], np.arange(k + 1))
    for j in range(k):
        if bounds[j + 1] > bounds[j]:
            out[j] = np.median(X[order[bounds[j]:bounds[j + 1]]], axis=0)
    return out


def sort_medians(X: np.ndarray, lab: np.ndarray, k: int) -> np.ndarray:
    """The contract at the top of csrc/medians.hip, from the sorted values:
    ((0.0 + s[(m-1)//2]) + s[m//2]) / 2, or (0.0 + s[m//2]) / 1 for odd m."""
    out = np.full((k, X.shape[1]), np.nan)
    for j in range(k):
        rows = X[lab == j]
        m = rows.shape[0]
        if m == 0:
            continue
        s = np.sort(rows, axis=0)
        if m & 1:
            out[j] = (0.0 + s[m // 2]) / 1.0
        else:
            out[j] = ((0.0 + s[(m - 1) // 2]) + s[m // 2]) / 2.0
    return out


# ---- the named cases -------------------------------------------------------
def _split(n: int, k: int, seed: int) -> np.ndarray:
    """k uneven positive sizes summing to n."""
    rng = np.random.default_rng(seed)
    w = rng.random(k) + 0.2
    s = np.maximum(1, np.floor(w / w.sum() * (n - k)).astype(np.int64))
    s[0] += n - s.sum()
    assert s.sum() == n and s.min() >= 1
    return s


BLOCK_N = (MG_BLOCK - 1, MG_BLOCK, MG_BLOCK + 1, MG_BLOCK * MG_RANGE, MG_BLOCK * MG_RANGE + 1,
           2 * MG_BLOCK * MG_RANGE + MG_BLOCK + 1)
BIG_K = ((257, 3), (1025, 3), (1500, 17), (2049, 3))          # (k, d)
LANE_D = (1, 2, 3, 5, 64, 65, 127, 128)
MODES = ("f32x", "f64")
PART_SIZES = (600, 500, 301, 2, 1)
PART_D = 8


# sharded passes: rows of cluster j on shard s
# cluster:        0         1        2     3    4   5
TWO_SHARDS = ((40, 51, 7, 0, 1, 0),      # shard 0
              (61, 49, 0, 64, 0, 0))     # shard 1
THREE_SHARDS = ((3000, 2500, 1, 411, 0), (17, 0, 300, 2, 0), (0, 4, 0, 1, 0))
# name -> (sizes, d, seed): the small sets of the sharded and the stale-state tests
_SMALL = {
    "shards2": (np.sum(TWO_SHARDS, axis=0), 3, 52),
    "shards3": (np.sum(THREE_SHARDS, axis=0), 3, 53),
    "mixed": ((301, 200, 77, 6), 4, 54),
    "stale_a": ((500, 300, 211), 4, 55),
    "stale_b": ((500, 300, 211), 4, 56),
}


def lane_sizes(d: int):
    R = hist_rows(d)
    return (1, 2, R - 1, R, R + 1, MG_U * R + 1)


def part_plants(mode: str, seed: int):
    """The planted columns of the "where the ranks part" case, each with what
    its two middle values are: (cluster, feature, values, note)."""
    rng = np.random.default_rng(seed)
    f32 = mode == "f32x"
    nxt = (float(np.nextafter(np.float32(0.5), np.float32(1.0))) if f32
           else float(np.nextafter(0.5, 1.0)))
    m0, m1, m2 = PART_SIZES[:3]
    out = []
    # cluster 0 (anchor 0: the ball crosses zero)
    out.append((0, 0, column(m0, 0.0, [0.125, 0.125], mode), "equal"))
    out.append((0, 1, column(m0, 0.0, [-0.25, 0.25], mode), "opposite sign"))
    j, lo, hi = byte_pair(0, mode, rng)
    assert j == 0
    out.append((0, 2, column(m0, 0.0, [lo, hi], mode), "byte 0"))
    z = np.zeros(m0)
    z[::3] = -0.0
    out.append((0, 3, z, "zeros"))
    out.append((0, 4, column(m0, 0.0, [0.375] * 100, mode), "ties"))
    out.append((0, 5, column(m0, 0.0, [0.5, nxt], mode), "neighbours"))
    out.append((0, 6, column(m0, 0.0, [-0.0, 0.0], mode), "signed zeros in the middle"))
    # cluster 1 (anchor 4): every lower key byte
    nbytes = 4 if f32 else 8
    for p in range(1, nbytes):
        j, lo, hi = byte_pair(p, mode, rng)
        assert j == 1
        out.append((1, p - 1, column(m1, 4.0, [lo, hi], mode), "byte %d" % p))
    out.append((1, 7, column(m1, 4.0, [4.5, 4.5, 4.5, 4.5], mode), "ties"))
    # cluster 2 (odd size): a tie run around the one middle rank
    out.append((2, 0, column(m2, 8.0, [8.25] * 51, mode), "ties, odd"))
    return out


def _spec(name: str):
    kind, *rest = name.split("-")
    mode = rest[-1]
    if kind == "blocks":
        n = int(rest[0])
        return _split(n, 7, n), 2, mode, n % 1000, ()
    if kind == "bigk":
        k, d = int(rest[0]), int(rest[1])
        sizes = np.random.default_rng(k).integers(1, 17, k)
        return sizes, d, mode, k + d, ()
    if kind == "lanes":
        d = int(rest[0])
        return lane_sizes(d), d, mode, 100 + d, ()
    if kind == "part":
        return PART_SIZES, PART_D, mode, 7, [p[:3] for p in part_plants(mode, 11)]
    if kind in _SMALL:
        sizes, d, seed = _SMALL[kind]
        return sizes, d, mode, seed, ()
    if kind == "builder":     # checked on the CPU only
        d, k = int(rest[0]), int(rest[1])
        sizes = np.random.default_rng(d * k).integers(0, 6, k)
        return sizes, d, mode, d + k, ()
    raise KeyError(name)


CASES = tuple(
    ["blocks-%d-%s" % (n, m) for n in BLOCK_N for m in MODES]
    + ["bigk-%d-%d-%s" % (k, d, m) for k, d in BIG_K for m in MODES]
    + ["lanes-%d-%s" % (d, m) for d in LANE_D for m in MODES]
    + ["part-%s" % m for m in MODES]
    + ["%s-%s" % (nm, m) for nm in ("shards2", "shards3") for m in MODES]
    + ["mixed-f32x", "stale_a-f32x", "stale_b-f32x", "stale_a-f64"])
BUILDER_ONLY = tuple("builder-%d-%d-%s" % (d, k, m)
                     for d, k in ((1, 1500), (3, 2049), (70, 40), (5, 300)) for m in MODES)


@functools.lru_cache(maxsize=4)
def case(name: str):
    """(X, C, labels, sizes) of a named case; the arrays are read-only."""
    sizes, d, mode, seed, plants = _spec(name)
    X, C, lab = labelled_points(sizes, d, mode, seed, plants)
    for a in (X, C, lab):
        a.setflags(write=False)
    return X, C, lab, np.asarray(sizes, dtype=np.int64)

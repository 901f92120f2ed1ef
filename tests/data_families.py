"""Data families outside the unit cube (TEST INFRASTRUCTURE ONLY).

Every other parity test feeds the storage-mode decision (decide_mode,
csrc/cdr_runtime.hip) features in [0, 1) on the 2^-24 grid or min-max
normalised doubles.  These families move, stretch and mix the ranges, the
grid and the sign so that the scale S, the screen transform (mu, sigma) and
the exactness of the pre-centred copy (pre_ok) all leave their usual values.

``family(name, n, d, seed)`` builds X from ``g = synth.generate(n, 0, n, d,
40, seed)``; ``EXPECT`` holds what the gate has to answer for each family;
``CASES`` are the (family, n, d, k) the tests run and ``reference`` the
oracle's results for one of them, computed once per process.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import kmeans_oracle as ko
from oracle import synth

MODE_F32X, MODE_F64 = 1, 2

# name -> (mode, scale_bits, pre_ok); None = not asserted.
#  offset      |x| ~ 1000 on the 2^-14 grid: 24 significant bits, mu far from 0
#  int_signed  whole numbers in [-2^19, 2^19): S = 0, negative minimum
#  mixed       ranges 1 and 4096 side by side: sigma = -11 for every feature
#  wide_int    multiples of 64 below 2^29: S = 0, but |x - mu| reaches 2^28
#              units, beyond the 2^24 an exact fp32 pre-centred copy allows
#  outlier     one row at 32 - 2^-19 next to [0, 1) data on the 2^-24 grid:
#              sigma = -5 and |x - mu| ~ 2^28 grid steps
#  const_dup   two constant columns (range 0) and every row twice
#  tiny        fp32 subnormals on the 2^-140 grid: S would be 140, and 2^140 is
#              no finite float (the mode is reported, not asserted)
#  small       the finest grid the gate keeps in F32X: S = 126, every non-zero
#              |x| a normal float (>= 2^-126), 2^S a finite one
#  big_f64     fp32-exact whole numbers up to 2^50: past the |x| 2^S < 2^30 gate
#  raw_f64     unnormalised doubles, scales 1e-3 .. 1e9, odd columns signed
EXPECT = {
    "offset": (MODE_F32X, 14, True),
    "int_signed": (MODE_F32X, 0, True),
    "mixed": (MODE_F32X, 12, True),
    "wide_int": (MODE_F32X, 0, False),
    "outlier": (MODE_F32X, 24, False),
    "const_dup": (MODE_F32X, 24, True),
    "tiny": None,
    "small": (MODE_F32X, 126, True),
    "big_f64": (MODE_F64, 0, None),
    "raw_f64": (MODE_F64, 0, None),
}
FAMILIES = tuple(EXPECT)
F32_EXACT = FAMILIES[:-1]  # every family but raw_f64 survives a float32 round trip

_RAW_SCALES = (1e6, 1.0, 1e-3, 3600.0, 1e9)


def _minmax(rng, n, d):
    """Min-max normalised doubles with full 53-bit mantissas (as in
    test_gpu_f64_update.py)."""
    raw = rng.gamma(2.0, 3.0, (n, d)) * rng.random(d) + rng.normal(0, 1, (n, d))
    return (raw - raw.min(axis=0)) / (raw.max(axis=0) - raw.min(axis=0))


def family(name: str, n: int, d: int, seed: int) -> np.ndarray:
    g = synth.generate(n, 0, n, d, 40, seed)
    if name == "offset":
        return 1000.0 + np.floor(g * 2.0 ** 14) / 2.0 ** 14
    if name == "int_signed":
        return np.floor(g * 2.0 ** 20) - 2.0 ** 19
    if name == "mixed":
        X = np.floor(g * 2.0 ** 12) / 2.0 ** 12
        X[:, 0::3] = np.floor(g[:, 0::3] * 2.0 ** 24) / 2.0 ** 12
        return X
    if name == "wide_int":
        return np.floor(g * 2.0 ** 23) * 64.0
    if name == "outlier":
        X = g.copy()
        X[n // 2] = 32.0 - 2.0 ** -19
        return X
    if name == "const_dup":
        X = g.copy()
        X[:, 1] = 0.375
        X[:, -1] = 0.0
        m = n // 2
        X[1:2 * m:2] = X[0:2 * m:2]
        return X
    if name == "tiny":
        return np.ldexp(np.floor(g * 2.0 ** 20), -140)
    if name == "small":
        return np.ldexp(np.floor(g * 2.0 ** 20), -126)
    if name == "big_f64":
        return np.floor(g * 2.0 ** 20) * 2.0 ** 30
    if name == "raw_f64":
        X = _minmax(np.random.default_rng(seed), n, d)
        for f in range(d):
            s = _RAW_SCALES[f % 5]
            X[:, f] *= s
            if f % 2:
                X[:, f] -= 0.5 * s
        return X
    raise KeyError(name)


SHAPES_ALL = (24_001, 16, 64)
# screen32 QH1/MT1; the host-plan screens: screen_kernel (k = 33: three
# 16-centroid tiles x two 16-feature chunks) and screen_fast (k = 20: two x
# two, the most it takes); large k
SHAPES_F32X = ((16_500, 5, 7), (20_000, 24, 33), (18_000, 24, 20), (12_000, 32, 300))
SEED_RANDOM_STATE = 7

# (family, n, d, k): every family at the screen32 shape; the four that move
# the gate the most at the other shapes.
CASES = [(name,) + SHAPES_ALL for name in FAMILIES] + [
    (name,) + s for s in SHAPES_F32X
    for name in ("offset", "int_signed", "wide_int", "outlier")] + [
    # with S = 140 kept as F32X, this shape's screen_fast step scaled by
    # 2^140 = inf as a float and returned wrong sums (the screen32 shape did not)
    ("tiny", 18_000, 24, 20)]

# Data seed of a case; a pair whose oracle run leaves a cluster empty or
# draws a row twice gets another seed here (the family stays as it is).
_SEEDS: dict[tuple, int] = {
    ("offset", 20_000, 24, 33): 157,  # (57 empties a cluster in the first step)
}


def case_id(case) -> str:
    return "%s-%dx%d-k%d" % case


def data_seed(case) -> int:
    name, n, d, k = case
    return _SEEDS.get(case, 1000 * FAMILIES.index(name) + d + k)


def loop_steps(k: int) -> int:
    return 3 if k >= 300 else 4


@functools.lru_cache(maxsize=None)
def data(case) -> np.ndarray:
    name, n, d, k = case
    X = family(name, n, d, data_seed(case))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference(case) -> dict:
    """The oracle on one case: k-means++ seeds C0 (random_state 7), then
    ``loop_steps(k)`` Lloyd steps from them exactly as
    ``ko.lloyd(X, C0, steps, -1.0)`` takes them (same assign and update calls),
    keeping every step's labels.  Shared by the CPU and the GPU tests and
    never written to."""
    name, n, d, k = case
    X = data(case)
    C0 = ko.kmeans_plusplus_init(X, k, random_state=SEED_RANDOM_STATE)
    C, labels = C0, []
    for _ in range(loop_steps(k)):
        lab = ko.assign(X, C)
        labels.append(lab)
        C = ko.update(X, lab, C, n)
    for a in [C0, C] + labels:
        a.setflags(write=False)
    return {"C0": C0, "C": C, "labels": labels}

"""Designed inputs for the large-k Lloyd path, csrc/screen_big.hip (TEST
INFRASTRUCTURE ONLY; no GPU, nothing from the device library).

``case(d, k)`` returns ``(X, C, expect)`` for one shape of ``SHAPES``: bulk rows
of ``synth.generate`` plus designed points, and k start centroids that are bulk
rows except at the designed indices.  Every value of X and C is a multiple of
2^-10 inside [0, 1), so the load stays F32X with exact pre-centring.  A
designed site is a random location with every coordinate in [0.2, 0.8], drawn
again until it is more than 0.32 from every bulk row and 0.55 from every other
site, while everything designed happens within 0.2 of its site: with
|delta|^2 = 0.0149 every other centroid is more than 0.087 farther in the
squared distance than the designed ones.
``expect`` holds, per designed point, the row in X, the label the reference
must give and the level of the path meant to decide it (1: L1 certifies it,
2: L2 with at most kMaxCand candidates, 3: L3, 0: not designed for a level),
and per pair the two centroid indices and whether the roots tie.
tests/test_big_cases.py checks all of it with the oracle alone.

What is designed (delta has two non-zero coordinates, 96 and 80 grid units:
|delta| = 0.122, about 2^-3):

* exact ties: point x, centroids x + delta and x - delta at the indices
  (j1, j2): the squared terms are the same numbers, the fp64 roots are equal
  and the first index wins.  The index pairs are placed inside one 32-block in
  one lane half (only the low 4 index bits differ), across the halves of one
  block, in two blocks, across the index edges 31|32, 1023|1024, 2047|2048 and
  4095|4096 where k reaches them, with the winner at j = 0, and with the
  winner at j = k - 1 in a padded last block (k % 32 != 0);
* near ties: the same geometry with one coordinate of one centroid moved by
  one grid unit, so the squared distances differ by 191 * 2^-20 = 1.8e-4, far
  below the screen's threshold T1 (>= 8e-3 at d = 9, see csrc/screen_big.hip
  big_bounds): "near-hi" moves the higher-indexed centroid closer, "near-lo"
  moves the lower-indexed one away; the higher index wins both;
* every placement with room for four index pairs carries the four variants
  tie with the lower index at +delta, tie with it at -delta, near-hi, near-lo;
  the winner-at-0 pair is a tie in the order the shape's parity picks, the
  winner-at-(k-1) pair is near-hi;
* candidate clusters: m = 2, 15, 16, 17 and 40 centroids within one grid unit
  of a location, at random indices; the second-lowest index and the fourth sit
  exactly on the location, the lowest does not, the highest duplicates the
  third; two points on the location and one on every centroid.  m <= 16 is
  decided in L2, m >= 17 overflows to L3; the first index of the duplicates
  must win in both;
* eviction pairs: a tie whose winner j1 also owns three points at
  x + 1.5 delta.  The mean of that cluster is x + 1.125 delta, so in the next
  step x is 1.2656 |delta|^2 from j1 and |delta|^2 from j2 (a gap of 4e-3,
  below T1): x changes label in every step of the sequence below, unless a
  bulk row joins one of the two clusters and shifts its mean (four such pairs:
  tests/test_big_cases.py asks that some of them move in every step);
* solo centroids: a centroid alone at its site with four points within one
  grid unit: certified by L1.

``sequence(d, k)`` is the four-step sequence of the host-plan delta test: C,
the means of the result, C with the rows of the first solo centroid and of the
17-cluster's winner swapped, the means again.  The swap moves a solo cluster
(L1 moves) and, unless a duplicate has taken them over in the means step
before, the points on the 17-cluster's location (L3 moves); eviction pairs
move in every step (L2 moves).  An empty cluster keeps its
centroid.  The only empty clusters are the later copies of exact duplicate
centroids, which can never win a point.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import kmeans_oracle as ko
from oracle import synth

GRID_BITS = 10
UNIT = 2.0 ** -GRID_BITS
KMAXCAND = 16                 # kMaxCand of csrc/screen_big.h
CLUSTER_M = (2, 15, 16, 17, 40)
DELTA = (96, 80)              # grid units in two coordinates
EDGES = (32, 1024, 2048, 4096)
SITE_CLEAR = 0.32            # a site's distance to every bulk row, at least

# (d, k) -> n: the form matrix of tests/test_gpu_screen_big.py
SHAPES = {(64, 1100): 4000, (40, 1500): 5000, (20, 2200): 6000, (12, 4200): 8000,
          (9, 2300): 6000, (24, 1200): 5000, (64, 1152): 4000, (12, 4256): 8000,
          (33, 1025): 4000}


def form(d: int, k: int) -> dict:
    """The form the host code of csrc/screen_big*.hip picks for (d, k), from the
    formulas of its big_supported, big_launch and the levels' launchers."""
    DQ, KB = -(-d // 16), -(-k // 32)
    lds1 = KB * 128 + KB * DQ * 1024
    fg = next((g for g in (16, 8, 4) if k * (g * 8 + 4) <= 150 * 1024), 0)
    JB = 5
    while (1 << (JB - 5)) < KB:
        JB += 1
    return {"DQ": DQ, "KB": KB, "FG": fg, "JB": JB, "l1_threads": 768 if DQ <= 2 else 512,
            "l2_form": 0 if lds1 + 8 * 64 * 4 + 8 * 64 * KMAXCAND * 2 <= 160 * 1024 else 1,
            "supported": 8 <= d <= 64 and lds1 <= 150 * 1024 and fg > 0}


def pair_slots(k: int):
    """[(placement, [(j1, j2), ...])]: the index pairs of the ties, j1 < j2 < k.
    Four pairs (one per variant) where the placement has room for them."""
    KB = -(-k // 32)
    slots = []
    if k % 32:
        slots.append(("last", [(k - 3, k - 1)]))
    slots.append(("first", [(0, 7)]))
    slots.append(("half", [(97, 102), (98, 105), (99, 108), (100, 111)]))
    slots.append(("halves", [(161, 177), (162, 185), (167, 176), (175, 191)]))
    slots.append(("blocks", [(7 * 32 + 3, 9 * 32 + 3), (7 * 32 + 5, 11 * 32 + 20),
                             (8 * 32, 20 * 32 + 31), (10 * 32 + 9, (KB - 2) * 32 + 9)]))
    for e in EDGES:
        slots.append(("edge%d" % e, [(e - 1 - i, e + i) for i in range(4) if e + i < k]))
    return slots


VARIANTS = ("tie+", "tie-", "near-hi", "near-lo")


def _pair(x, f0, f1, variant):
    """Grid-unit centroids (c_j1, c_j2) around x and the winner (0: j1, 1: j2)."""
    dl = np.zeros_like(x)
    dl[f0], dl[f1] = DELTA
    plus, minus = x + dl, x - dl
    if variant == "tie+":
        return plus, minus, 0
    if variant == "tie-":
        return minus, plus, 0
    if variant == "near-hi":      # the higher index one unit closer
        minus[f0] += 1
        return plus, minus, 1
    minus[f0] -= 1                # near-lo: the lower index one unit farther
    return minus, plus, 1


def build(d: int, k: int, n: int, seed: int, dups: bool = True):
    """(X, C, expect) as the module docstring describes.  ``dups=False``
    replaces the exact duplicate centroids of the clusters by further distinct
    offsets (no cluster of the start centroids is empty then)."""
    rng = np.random.default_rng(seed)
    Cg = np.zeros((k, d), dtype=np.int64)
    taken = np.zeros(k, dtype=bool)
    rows, labels, levels, kinds = [], [], [], []
    pairs = []   # (index into rows, j1, j2, tie, placement, variant)

    # bulk rows floored to the grid (the first nb of them are used)
    bulk = np.floor(synth.generate(n, 0, n, d, k, seed) * 2.0 ** GRID_BITS).astype(np.int64)
    sites = []

    def site():
        # more than SITE_CLEAR from every bulk row and 0.55 from every other site
        for _ in range(5000):
            x = rng.integers(205, 820, d)
            if (np.sqrt(((bulk - x) ** 2).sum(axis=1).min()) * UNIT > SITE_CLEAR and
                    all(np.sqrt(((s - x) ** 2).sum()) * UNIT > 0.55 for s in sites)):
                sites.append(x)
                return x
        raise RuntimeError("no room for another designed site")

    def point(x, label, level, kind):
        rows.append(np.array(x, dtype=np.int64))
        labels.append(int(label))
        levels.append(level)
        kinds.append(kind)
        return len(rows) - 1

    def put_pair(j1, j2, variant, placement, evict=False):
        assert j1 < j2 < k and not taken[j1] and not taken[j2], (j1, j2, k)
        x = site()
        f0, f1 = rng.choice(d, 2, replace=False)
        c1, c2, win = _pair(x, f0, f1, variant)
        Cg[j1], Cg[j2] = c1, c2
        taken[j1] = taken[j2] = True
        r = point(x, (j1, j2)[win], 2, ("evict " if evict else "") + placement + " " + variant)
        pairs.append((r, j1, j2, variant.startswith("tie"), placement, variant))
        if evict:   # the winner's cluster is pulled away from x
            for _ in range(3):
                point(x + 3 * (c1 - x) // 2, j1, 0, "evict support")
        else:
            point(c1, j1, 0, "pair support")
        for _ in range(3 if evict else 1):
            point(c2, j2, 0, "pair support")

    for placement, idx in pair_slots(k):
        idx = [p for p in idx if not taken[p[0]] and not taken[p[1]]]
        if placement == "last":
            put_pair(*idx[0], "near-hi", placement)
        elif placement == "first":
            put_pair(*idx[0], VARIANTS[(d + k) & 1], placement)
        else:
            for v, (j1, j2) in enumerate(idx):
                put_pair(j1, j2, VARIANTS[v], placement)

    def free(m):
        return np.sort(rng.choice(np.flatnonzero(~taken), m, replace=False))

    for v in range(4):   # eviction pairs, in two blocks
        j1, j2 = free(2)
        put_pair(int(j1), int(j2), VARIANTS[v & 1], "free", evict=True)

    winners = {}
    for m in CLUSTER_M:
        idx = free(m)
        taken[idx] = True
        L = site()
        codes = rng.choice(np.arange(1, 1 << 9), m, replace=False)   # distinct non-zero 0/1 offsets
        offs = [np.array([(int(c) >> f) & 1 if f < 9 else 0 for f in range(d)]) for c in codes]
        if m == 2:
            offs[1] = 0 * offs[1]
            if dups:
                offs[0] = 0 * offs[0]
        else:
            offs[1] = 0 * offs[1]
            if dups:
                offs[3] = 0 * offs[3]
                offs[m - 1] = offs[2]
        for j, o in zip(idx, offs):
            Cg[j] = L + o
        level = 2 if m <= KMAXCAND else 3

        def first(o):
            return int(next(j for j, q in zip(idx, offs) if np.array_equal(q, o)))

        winners[m] = first(0 * offs[0])
        for _ in range(2):
            point(L, winners[m], level, "cluster %d location" % m)
        for o in {tuple(o) for o in offs}:
            point(L + np.array(o), first(np.array(o)), level, "cluster %d centroid" % m)

    solos = [int(j) for j in free(2)]
    for j in solos:
        taken[j] = True
        L = site()
        Cg[j] = L
        for t in range(4):
            o = np.zeros(d, dtype=np.int64)
            if t:
                o[rng.integers(0, d)] = (-1) ** t
            point(L + o, j, 1, "solo")

    # the other centroids are bulk rows
    nb = n - len(rows)
    bulk = bulk[:nb]
    rest = np.flatnonzero(~taken)
    assert nb >= rest.size, (n, k)
    Cg[rest] = bulk[np.sort(rng.choice(nb, rest.size, replace=False))]
    Xg = np.concatenate([bulk, np.array(rows)])
    perm = rng.permutation(n)   # the designed rows spread over the waves
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    X = np.ascontiguousarray(Xg[perm] * UNIT)
    C = Cg * UNIT
    expect = {"rows": inv[nb:], "labels": np.array(labels), "levels": np.array(levels),
              "kinds": kinds, "winners": winners, "solos": solos,
              "pairs": [(int(inv[nb + r]), j1, j2, tie, pl, v) for r, j1, j2, tie, pl, v in pairs]}
    return X, C, expect


@functools.lru_cache(maxsize=None)
def case(d: int, k: int, dups: bool = True):
    X, C, expect = build(d, k, SHAPES[(d, k)], 1000 * d + k, dups)
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C, expect


def means(X, labels, C):
    """The next centroids: the mean of every cluster; an empty one keeps its row."""
    k = C.shape[0]
    cnt = np.bincount(labels, minlength=k)
    s = np.zeros_like(C)
    np.add.at(s, labels, X)
    out = np.array(C)
    out[cnt > 0] = s[cnt > 0] / cnt[cnt > 0, None]
    return out


def swap_rows(C, expect):
    """C with the rows of the first solo centroid and the 17-cluster's winner swapped."""
    a, b = expect["solos"][0], expect["winners"][17]
    out = np.array(C)
    out[[a, b]] = out[[b, a]]
    return out


@functools.lru_cache(maxsize=None)
def sequence(d: int, k: int):
    """[(C_t, oracle labels_t)] for the four steps C, means, C swapped, means."""
    X, C, expect = case(d, k)
    steps = []
    C0 = np.array(C)
    lab = ko.assign(X, C0)
    steps.append((C0, lab))
    C1 = means(X, lab, C0)
    steps.append((C1, ko.assign(X, C1)))
    C2 = swap_rows(C0, expect)
    lab = ko.assign(X, C2)
    steps.append((C2, lab))
    C3 = means(X, lab, C2)
    steps.append((C3, ko.assign(X, C3)))
    for Ct, lt in steps:
        Ct.setflags(write=False)
        lt.setflags(write=False)
    return steps


def sums(X, labels, k, scale_bits):
    """The (k, d+1) int64 fixed-point sums and counts a device step returns."""
    out = np.zeros((k, X.shape[1] + 1), dtype=np.int64)
    np.add.at(out[:, :-1], labels, np.ldexp(X, scale_bits).astype(np.int64))
    out[:, -1] = np.bincount(labels, minlength=k)
    return out

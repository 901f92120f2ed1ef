"""Designed (cluster, feature) sequences for the exact sequential sums of
csrc/f64sum.hip, and a restatement of f64_walk (TEST INFRASTRUCTURE ONLY).

The suite's F64 data is min-max normalised random doubles.  On such data an
addition is an exact rounding tie about once in 5000 additions and almost
never after the first group of 64 blocks, the running value never lands on a
power of two, and no binade is subnormal: the odd-entry half of every
transfer (D1, P1, xc_compose's parity selection) and the limits of the
transfer test hardly run.  The families here put the running value where
those parts decide the result.

Layout of every case: ``X`` is (n, d); column 0 is a selector, 1000 (j + 1)
for a row of cluster j, ``C[j, 0]`` the same value and the rest of ``C`` zero,
so the assignment is known (``labels``; the tests still assert ko.assign).
Rows are dealt to the clusters at random, so every block holds members of
every cluster; the other columns carry the designed values in member order.

  pinned_ties   first member 2^20 + x, then odd multiples of 2^-p in [0.5, 1),
                p in 31..35 (the half-grid of binade 20 is 2^-33): one binade
                throughout, so whole groups and runs of groups apply composed,
                with ties inside and both entry parities
  growing_ties  the same values with p in 34..53 around the half-grid of the
                binade the running value has reached, no pin: the largest
                sequences (k = 2) cross binades 0..14, with ties at every level
  landings      column f is 1.0 for a cluster's first 2^(8 + f') members (f' =
                1 + (f - 1) mod 3), so the running value is exactly 2^(8 + f')
                there (m2 == kTop); then addends odd on the OLD binade's grid
                (every one a tie on the new grid), in [2^-6, 2^-5) so that
                few further crossings follow.  Cluster 0 has 16 members
                in every block, so its landings fall at the end of block 31
                (f' = 1: a block end inside group 0) and of blocks 63 / 127
                (f' = 2, 3: group ends); the other clusters' fall mid-block
  tiny          whole multiples of 2^-1074 below 2^-1018, small first: the
                running value is subnormal for many blocks (no fixed grid:
                kMinE), passes 2^-1022 and goes on through normal binades
  signs         sequence (j, f) number t = j (d - 1) + f - 1:  t = 0 cancels
                to exactly +0.0 at member 300, stays there over a block start
                and goes on with fine-grained small addends;  t = 1 starts
                with five -0.0 members;  t = 2 is
                pinned at -2^20 (a negative running value throughout);  the
                others are pinned_ties with a negative addend every 1000
                members, sized so that the running value dips below 2^20 and
                climbs back (single flagged blocks, a crossing after each)
  large         pinned_ties with the designed columns scaled by 2^500 (xfer_pre's
                ldexp(x, MB - e) at a large e).  The squared distances overflow,
                so NumPy assigns every row to cluster 0: ``labels`` is all zero
  large_sel     pinned_ties with the whole case (selector and C too) scaled by
                2^480: the assignment stays known, every sequence sits in
                binade 500 with ties
  large_inf     the designed columns scaled by 2^1003: the second pin makes
                the column sum inf (all rows in cluster 0, as for large)
  f32_*         pinned_ties / growing_ties for a 24-bit significand, float32
                input: pin 2^10 with p in 12..14 (half-grid 2^-14), or values
                in [128, 256) with p around 24 - e.  "_x": on the 2^-14 grid,
                stored F32X (sums_parallel<float, float>); "_d": p up to 16,
                past the gate's |x| 2^S < 2^30, stored as doubles
                (sums_parallel<float, double>)
  minmax        min-max normalised random doubles in the same layout: what the
                other tests feed this path (for the printed comparison)

``model_walk`` restates f64_walk with the running value's own binade in place
of the device's prediction from approximate prefix sums (a prediction can
only miss near a crossing, where the device then walks one more block).
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

import f64prog_model as fm

KFB = fm.KFB
GROUP = 64
F64 = (52, -1022)   # (MB, kMinE) of SumTraits<double>
F32 = (23, -126)    # SumTraits<float>

# (d, k) of the product forms: the fused step's three f64_transfer state
# widths (k <= 16, <= 32, <= 64), the separate passes (d > 16), the serial
# kernel (k > 64)
SHAPES = ((3, 2), (5, 20), (4, 40), (17, 3), (3, 70))
N_SMALL = 3 * 16384 + 77
N_BIG = 6 * 16384 + 300
N_OF = {"pinned_ties": N_SMALL, "growing_ties": N_BIG, "landings": N_BIG,
        "tiny": 2 * 16384 + 77, "signs": N_BIG, "large": N_SMALL, "large_sel": N_SMALL,
        "large_inf": N_SMALL, "minmax": N_BIG}
F64_FAMILIES = ("pinned_ties", "growing_ties", "landings", "tiny", "signs", "large",
                "large_sel", "large_inf")
# The same designed values and labels as a family, with one thing changed:
#  pinned_run / signs_run  the selector is 10^6 (j + 1).  Against a 2^20 pin
#                a spacing of 1000 does not hold the pin rows once the
#                centroids are means (2 * 2^20 * the clusters' difference in a
#                mean exceeds 1000^2), and at k >= 20 a cluster runs empty two
#                steps later; 10^12 outweighs it (differences in a mean stay
#                below 1000), so every Lloyd step keeps every label
#  signs_prog    sequence 2 (negative throughout, one ELEM item per member in
#                a sharded program) is a fourth-kind sequence instead, so the
#                sharded programs fit and run on flagged blocks
#  minmax_small  minmax at pinned_ties' n
VARIANT_OF = {"pinned_run": "pinned_ties", "signs_run": "signs", "signs_prog": "signs",
              "minmax_small": "minmax"}
# float32 cases: name -> (n, d, k, expected storage mode)
F32_CASES = {"f32_pinned_x": (45_077, 4, 40, 1), "f32_pinned_d": (45_077, 4, 40, 2),
             "f32_growing_x": (N_BIG, 5, 20, 1), "f32_growing_d": (N_BIG, 5, 20, 2)}

# Mutants of the model and the family built to catch each.  Two further
# changes to the kernel are not among them because they cannot change any sum:
#  * "<=" for "<" at the binade's top (m2 == kTop accepted): the transfer then
#    says the running value is exactly 2^(e+1).  Every step before was below
#    kTop, where the grid arithmetic is the real rounding, and a step that
#    reaches kTop on the grid of binade e also rounds to 2^(e+1) in fp64 (the
#    exact sum is below kTop + 1/2, or a tie that goes to the even 2^(e+1));
#    addends after it that leave m at kTop are at most half a step of the old
#    grid, which the coarser new grid drops as well.  The value written,
#    ldexp(kTop, e - MB), is therefore the right one, and the next block is
#    judged in the new binade either way.  (landings still runs that case.)
#  * subnormal binades accepted (no kMinE test): below 2^kMinE every value is
#    a whole multiple of the smallest subnormal, so the additions are exact in
#    fp64 and exact in a transfer on any finer grid: both give the same sum.
MUTANTS = {"entry": "pinned_ties", "exit": "pinned_ties", "tie_up": "growing_ties",
           "neg_ok": "signs", "zero_ok": "signs"}

Walk = namedtuple("Walk", "sum ties blocks groups walked")


def _compose(a, b, mutant=None):
    if mutant == "entry":  # the second transfer's entry parity ignored
        p = b[2] & 1
        return a[0] + b[0], a[1] + b[0], p | (p << 1)
    return fm.compose(a, b)


class _Seq:
    """One sequence's members by row-block, with the per-block transfers in a
    binade e formed for all blocks at once (cached per e)."""

    def __init__(self, col, labels, j, fmt, mutant):
        idx = np.flatnonzero(labels == j)
        self.vals = np.asarray(col[idx], dtype=np.float64)
        nb = -(-col.size // KFB)
        self.nb = nb
        self.start = np.searchsorted(idx // KFB, np.arange(nb + 1))
        self.live = np.flatnonzero(np.diff(self.start) > 0)
        self.mb = fmt[0]
        self.mutant = mutant
        self._cache = {}

    def block(self, b):
        return self.vals[self.start[b]:self.start[b + 1]]

    def _tables(self, e):
        t = self._cache.get(e)
        if t is None:
            mb, v = self.mb, self.vals
            with np.errstate(over="ignore", invalid="ignore"):
                y = np.ldexp(v, mb - e)
                qf = np.floor(y)
                fr = y - qf
            bad = np.isnan(v) | ~(y < 2.0 ** (mb + 1)) | ~(y > -2.0 ** 62)
            if self.mutant != "neg_ok":
                bad |= ~(v >= 0.0)
            q = np.where(bad, 0.0, qf).astype(np.int64)
            tie = (fr == 0.5) & ~bad
            inc = np.where(tie, 0, q + (fr > 0.5))
            at = self.start[self.live]
            t = (q, tie, inc, np.add.reduceat(inc, at), np.add.reduceat(tie.astype(np.int64), at),
                 np.add.reduceat(bad.astype(np.int64), at))
            self._cache[e] = t
        return t

    def xfer(self, li, e):
        """(d0, d1, p, ties) of live block number li in binade e, or None
        (xfer_pre's invalid flag: a negative or non-finite addend, or one not
        below the binade's top)."""
        q, tie, inc, dsum, ntie, nbad = self._tables(e)
        if nbad[li]:
            return None
        if not ntie[li]:
            dd = int(dsum[li])
            p0 = dd & 1
            return dd, dd, p0 | ((p0 if self.mutant == "exit" else 1 ^ p0) << 1), 0
        b = self.live[li]
        s0, s1 = self.start[b], self.start[b + 1]
        pre = np.cumsum(inc[s0:s1])
        at = np.flatnonzero(tie[s0:s1])
        out = []
        for p in (0, 1):
            extra = 0
            for t in at:
                qt = int(q[s0 + t])
                if self.mutant == "tie_up":   # ties round away
                    extra += qt + 1
                else:                         # to even: m + q is odd -> up
                    extra += qt + ((p + int(pre[t]) + extra + qt) & 1)
            out.append(int(pre[-1]) + extra)
        p0, p1 = out[0] & 1, (1 + out[1]) & 1
        if self.mutant == "exit":             # P1 taken from P0
            p1 = p0
        return out[0], out[1], p0 | (p1 << 1), int(ntie[li])


def model_walk(col, labels, j, mutant=None, fmt=F64):
    """f64_walk for cluster j of one column: the first member's block element
    by element; then whole groups of 64 row-blocks composed (and runs of such
    groups) while they stay in the running value's binade; inside a group
    that does not, runs of blocks composed; a block whose transfer is flagged,
    whose running value has no binade (not positive, subnormal, not finite)
    or that would reach the binade's top is re-added in real arithmetic.
    Returns Walk(sum, ties inside applied transfers, blocks applied by
    transfer outside whole groups, groups applied whole, blocks walked)."""
    mb, mine = fmt
    top = 1 << (mb + 1)
    sq = _Seq(col, labels, j, fmt, mutant)
    s, any_ = 0.0, False
    ties = blocks = groups = walked = 0

    def cur_e():
        if not any_:
            return None
        if mutant == "zero_ok" and s == 0.0:
            return -1  # frexp(0) = (0, 0): the kernel's s > 0.0 test dropped
        e = fm.binade(s)
        return None if e is None or e < mine else e

    def stays(m, x):
        return m + (x[1] if m & 1 else x[0]) < top

    def apply(m, x, e):
        return math.ldexp(float(m + (x[1] if m & 1 else x[0])), e - mb)

    def run(first, last, e, unit):
        """The longest prefix of units first.. (each a list of live-block
        numbers) whose composed transfers keep the running value in binade e:
        (composed transfer, units taken, ties)."""
        m = int(math.ldexp(s, mb - e))
        acc, took, tt = None, 0, 0
        for u in range(first, last):
            cand, ct, ok = acc, 0, True
            for li in unit(u):
                x = sq.xfer(li, e)
                if x is None:
                    ok = False
                    break
                cand = x[:3] if cand is None else _compose(cand, x[:3], mutant)
                ct += x[3]
            if not ok or (cand is not None and not stays(m, cand)):
                break
            acc, took, tt = cand, took + 1, tt + ct
        return m, acc, took, tt

    ng = -(-sq.nb // GROUP)
    of_group = [[] for _ in range(ng)]
    for li, b in enumerate(sq.live):
        of_group[b // GROUP].append(li)
    g = 0
    while g < ng:
        if not of_group[g]:
            g += 1
            continue
        e = cur_e()
        if e is not None:
            m, acc, took, tt = run(g, ng, e, lambda u: of_group[u])
            if acc is not None:
                s = apply(m, acc, e)
                groups += sum(1 for u in range(g, g + took) if of_group[u])
                ties += tt
                g += took
                continue
        lis = of_group[g]
        i = 0
        while i < len(lis):
            e = cur_e()
            if e is not None:
                m, acc, took, tt = run(i, len(lis), e, lambda u: (lis[u],))
                if acc is not None:
                    s = apply(m, acc, e)
                    blocks += took
                    ties += tt
                    i += took
                    continue
            for v in sq.block(sq.live[lis[i]]).tolist():
                if not any_:
                    s, any_ = v, True
                elif mb == 52:
                    s = s + v
                else:
                    s = float(np.float32(s) + np.float32(v))
            walked += 1
            i += 1
        g += 1
    return Walk(s, ties, blocks, groups, walked)


# ---------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------
def odd_dyadic(rng, p, skew=1.0):
    """Odd multiples of 2^-p in [0.5, 1), one per entry of the int array p
    (2 <= p <= 53): an odd int64 below 2^53 through ldexp is exact.  skew > 1
    leans them towards 0.5, skew < 1 towards 1 (mean 0.5 + 0.5 / (skew + 1));
    an array gives every entry its own."""
    p = np.asarray(p, dtype=np.int64)
    half = np.ldexp(1.0, (p - 2).astype(np.int32))
    m = np.minimum(np.floor(half * (1.0 + rng.random(p.shape) ** skew)), 2.0 * half - 1.0).astype(np.int64)
    return np.ldexp((2 * m + 1).astype(np.float64), (-p).astype(np.int32))


def _ranks(labels, k):
    """Each row's rank among the rows of its cluster, and the cluster sizes."""
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=k)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.empty(labels.size, dtype=np.int64)
    rank[order] = np.arange(labels.size) - first[labels[order]]
    return rank, counts


def _growing_p(rng, rank, per_member, full, lo, hi):
    """p around the half-grid of the binade a running value of about
    per_member * rank has reached: full - e + (-2 .. 2), kept in lo..hi."""
    e = np.floor(np.log2(per_member * np.maximum(rank, 1))).astype(np.int64)
    return np.clip(full - e + rng.integers(-2, 3, rank.shape), lo, hi)


def _pinned(rng, rank, shape):
    V = odd_dyadic(rng, rng.integers(31, 36, shape))
    V[rank == 0] += 2.0 ** 20
    return V


def _landings_labels(rng, n, k):
    nb = n // KFB
    lab = np.empty(n, dtype=np.int64)
    for b in range(nb):
        blk = np.concatenate([np.zeros(16, dtype=np.int64), rng.integers(1, k, KFB - 16)])
        lab[b * KFB:(b + 1) * KFB] = rng.permutation(blk)
    lab[nb * KFB:] = rng.integers(1, k, n - nb * KFB)
    return lab


def landing_exponent(f):
    return 9 + (f - 1) % 3


def _signs_column(rng, t, m, nz):
    """Sequence number t of the signs family, m members; nz: members that
    span a whole row-block."""
    if t == 0:
        v = odd_dyadic(rng, _growing_p(rng, np.arange(m), 0.75, 53, 34, 53))
        z = min(300, m // 2)
        v[z] = -float(np.add.accumulate(v[:z])[-1])  # the running value: x + (-x) = +0.0
        # zeros to beyond the next block's start (a block that begins at a
        # running value of exactly 0), then 40 odd multiples of 2^-61 / 2^-62
        # below 2^-11, which a grid guessed from frexp(0) would round, then
        # odd multiples of 2^-62 below 2^-29 to the end: the sum stays near
        # 2^-6, where such an error is not rounded away again
        v[z + 1:z + 1 + nz] = 0.0
        w = min(m, z + 1 + nz + 40)
        v[z + 1 + nz:w] = np.ldexp(odd_dyadic(rng, rng.integers(50, 52, w - z - 1 - nz)), -11)
        v[w:] = np.ldexp(odd_dyadic(rng, np.full(m - w, 33)), -29)
        return v
    if t == 1:
        v = odd_dyadic(rng, _growing_p(rng, np.arange(m), 0.75, 53, 34, 53))
        v[:5] = -0.0
        return v
    v = odd_dyadic(rng, rng.integers(31, 36, m))
    if t == 2:
        v[0] = -(2.0 ** 20) - v[0]
        return v
    v[0] += 2.0 ** 20
    last = 1
    for i, at in enumerate(range(1000, m, 1000)):
        v[at] = -(np.rint(v[last:at].sum()) + (200.0 if i == 0 else 0.0))
        last = at + 1
    return v


@functools.lru_cache(maxsize=None)
def case(family, d, k):
    """{"X", "C", "labels" (the assignment the layout fixes), "sums" (NumPy's
    sequential sums under it)}, read-only and shared by the tests."""
    if family in F32_CASES:
        return _f32_case(family)
    variant, family = family, VARIANT_OF.get(family, family)
    n = N_SMALL if variant == "minmax_small" else N_OF[family]
    rng = np.random.default_rng(1000 * (1 + sorted(N_OF).index(family)) + 10 * d + k)
    lab = _landings_labels(rng, n, k) if family == "landings" else rng.integers(0, k, n)
    rank, counts = _ranks(lab, k)
    shape = (n, d - 1)
    rk = np.broadcast_to(rank[:, None], shape)
    if family in ("pinned_ties", "large", "large_sel", "large_inf"):
        V = _pinned(rng, rk, shape)
    elif family == "growing_ties":
        # A sequence walks one block per binade crossing outside its first
        # block, and the GPU tests bound the walked blocks: the first 256
        # members lean towards 1 (mean 0.9: more crossings inside the first
        # block), the others towards 0.5 (mean 0.6: the largest sequences,
        # n / 2 members, end in binade 14)
        V = odd_dyadic(rng, _growing_p(rng, rk, 0.6, 53, 34, 53), skew=np.where(rk < 256, 0.25, 4.0))
    elif family == "landings":
        ex = np.array([landing_exponent(f) for f in range(1, d)])
        # odd multiples of 2^(ex - 53) in [2^-6, 2^-5): few crossings afterwards
        V = np.ldexp(odd_dyadic(rng, np.broadcast_to(48 - ex, shape)), -5)
        V[rk < 2 ** ex] = 1.0
    elif family == "tiny":
        # odd counts of 2^-1074 with b bits, b up to 20 at a sequence's start
        # and up to 56 from its middle on
        bmax = np.clip(20 + (72 * rk) // np.maximum(counts[lab], 1)[:, None], 20, 56)
        b = 1 + np.floor(rng.random(shape) * bmax).astype(np.int64)
        V = np.ldexp(odd_dyadic(rng, np.maximum(b, 2)), (b - 1074).astype(np.int32))
        V[b == 1] = 2.0 ** -1074
    elif family == "signs":
        V = np.empty(shape)
        for j in range(k):
            rows = np.flatnonzero(lab == j)
            for f in range(1, d):
                t = j * (d - 1) + f - 1
                if t == 2 and variant == "signs_prog":
                    t = 3
                V[rows, f - 1] = _signs_column(rng, t, rows.size, 2 * (KFB // k) + 8)
    elif family == "minmax":
        from data_families import _minmax
        V = _minmax(rng, n, d - 1)
    else:
        raise KeyError(family)
    step = 1.0e6 if variant.endswith("_run") else 1000.0
    X = np.empty((n, d))
    X[:, 0] = step * (lab + 1)
    X[:, 1:] = V
    C = np.zeros((k, d))
    C[:, 0] = step * (np.arange(k) + 1)
    if family == "large":
        X[:, 1:] = np.ldexp(V, 500)
    elif family == "large_inf":
        X[:, 1:] = np.ldexp(V, 1003)
    elif family == "large_sel":
        X, C = np.ldexp(X, 480), np.ldexp(C, 480)
    if family in ("large", "large_inf"):
        lab = np.zeros(n, dtype=np.int64)  # every squared distance is inf: argmin takes 0
    return _freeze(X, C, lab, k)


def _f32_case(name):
    n, d, k, _ = F32_CASES[name]
    rng = np.random.default_rng(7000 + sorted(F32_CASES).index(name))
    lab = rng.integers(0, k, n)
    rank, _ = _ranks(lab, k)
    shape = (n, d - 1)
    rk = np.broadcast_to(rank[:, None], shape)
    pmax = 14 if name.endswith("_x") else 16
    if "pinned" in name:
        V = odd_dyadic(rng, rng.integers(12, pmax + 1, shape))
        V[rk == 0] = (V[rk == 0] + 2.0 ** 10).astype(np.float32)  # (the pin rounds to 24 bits)
    else:  # values in [128, 256): 8 + p significant bits
        V = np.ldexp(odd_dyadic(rng, 8 + _growing_p(rng, rk, 192.0, 24, 5, pmax)), 8)
    X = np.empty((n, d), dtype=np.float32)
    X[:, 0] = 1000.0 * (lab + 1)
    X[:, 1:] = V
    assert (X[:, 1:] == V).all()  # the designed values are float32 values
    C = np.zeros((k, d), dtype=np.float32)
    C[:, 0] = 1000.0 * (np.arange(k) + 1)
    return _freeze(X, C, lab, k)


def numpy_sums(X, labels, k):
    """np.add.reduce over each cluster's rows: row-sequential for d >= 2, in
    X's own dtype."""
    out = np.zeros((k, X.shape[1]), dtype=X.dtype)
    with np.errstate(over="ignore"):
        for j in range(k):
            m = labels == j
            if m.any():
                out[j] = np.add.reduce(X[m], axis=0)
    return out


def _freeze(X, C, lab, k):
    out = {"X": X, "C": C, "labels": lab, "sums": numpy_sums(X, lab, k)}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def walks(family, d, k, mutant=None):
    """model_walk of every designed sequence of a case: {(j, f): Walk}."""
    c = case(family, d, k)
    fmt = F32 if family in F32_CASES else F64
    X, lab = c["X"], c["labels"]
    return {(j, f): model_walk(X[:, f], lab, j, mutant, fmt)
            for j in np.unique(lab).tolist() for f in range(X.shape[1])}


def pairs(family, d, k):
    """(block, sequence) pairs of a case (the walked-block bound's base)."""
    n = case(family, d, k)["X"].shape[0]  # (every cluster present)
    return -(-n // KFB) * k * d

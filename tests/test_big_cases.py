"""The large-k case builder (tests/big_cases.py) builds what the GPU tests of
csrc/screen_big.hip rely on, checked with the oracle alone: designed ties are
exact ties of the fp64 roots, near ties are not, the oracle's labels are the
designed ones, every value is on the 2^-10 grid, and in the four-step
sequence of the host-plan delta test every step moves points, the designed
ones among them.  No GPU."""
import numpy as np
import pytest

import big_cases as bc
from oracle import kmeans_oracle as ko


def test_forms_are_the_ones_the_matrix_names():
    """The formulas of big_cases.form give the form each shape is in the
    matrix for, and the first unsupported k lies where the limits test puts it."""
    want = {(64, 1100): (4, 512, 1, 16, 11), (40, 1500): (3, 512, 1, 8, 11),
            (20, 2200): (2, 768, 1, 8, 12), (12, 4200): (1, 768, 1, 4, 13),
            (9, 2300): (1, 768, 0, 4, 12), (24, 1200): (2, 768, 0, 8, 11),
            (64, 1152): (4, 512, 1, 16, 11), (12, 4256): (1, 768, 1, 4, 13),
            (33, 1025): (3, 512, 0, 16, 11)}
    assert set(want) == set(bc.SHAPES)
    for (d, k), w in want.items():
        f = bc.form(d, k)
        assert f["supported"], (d, k)
        assert (f["DQ"], f["l1_threads"], f["l2_form"], f["FG"], f["JB"]) == w, (d, k, f)
        assert 4000 <= bc.SHAPES[(d, k)] <= 12000
    assert bc.form(33, 1025)["KB"] == 33 and bc.form(33, 1024)["JB"] == 10
    for d, k in [(64, 1152), (12, 4256)]:
        assert bc.form(d, k)["supported"] and not bc.form(d, k + 1)["supported"]
    assert not bc.form(7, 3000)["supported"]
    # the k bands of the global-memory L2 (cand_big) per DQ, in KB = ceil(k / 32)
    for d, lo, hi in [(64, 35, 36), (48, 46, 48), (32, 67, 70), (16, 127, 133)]:
        got = [kb for kb in range(1, 140)
               if bc.form(d, 32 * kb)["supported"] and bc.form(d, 32 * kb)["l2_form"] == 1]
        assert got == list(range(lo, hi + 1)), (d, got)
    assert [bc.form(8, k)["FG"] for k in (1163, 1164, 2258, 2259, 4266, 4267)] == [16, 8, 8, 4, 4, 0]


def _roots(x, C, js):
    return [float(np.sqrt(ko.sqdist_rows(x[None, :], C[j]))[0]) for j in js]


@pytest.mark.parametrize("d,k", sorted(bc.SHAPES))
def test_case_is_as_designed(d, k):
    X, C, ex = bc.case(d, k)
    n = bc.SHAPES[(d, k)]
    assert X.shape == (n, d) and C.shape == (k, d)
    for A in (X, C):   # on the grid, inside [0, 1)
        g = np.ldexp(A, bc.GRID_BITS)
        np.testing.assert_array_equal(g, np.rint(g))
        assert A.min() >= 0.0 and A.max() < 1.0
    steps = bc.sequence(d, k)
    lab = steps[0][1]
    np.testing.assert_array_equal(lab[ex["rows"]], ex["labels"])
    # the pairs: exact ties of the roots, or unequal roots; first index / nearer wins
    placements = set()
    for r, j1, j2, tie, placement, variant in ex["pairs"]:
        r1, r2 = _roots(X[r], C, (j1, j2))
        assert (r1 == r2) == tie, (placement, variant, r1, r2)
        assert lab[r] == (j1 if tie else j2)
        others = np.sqrt(ko.sqdist_rows(np.delete(C, (j1, j2), axis=0), X[r]))
        assert others.min() > bc.SITE_CLEAR, (placement, variant)
        placements.add((placement, variant))
        if placement == "half":
            assert j1 >> 4 == j2 >> 4
        elif placement == "halves":
            assert j1 >> 5 == j2 >> 5 and (j1 >> 4) + 1 == j2 >> 4
        elif placement == "blocks":
            assert j1 >> 5 != j2 >> 5
        elif placement.startswith("edge"):
            assert j1 < int(placement[4:]) <= j2
    for placement in ("half", "halves", "blocks", "edge32"):
        assert {v for p, v in placements if p == placement} == set(bc.VARIANTS), placement
    for e in bc.EDGES:
        if e + 3 < k:
            assert {v for p, v in placements if p == "edge%d" % e} == set(bc.VARIANTS)
    assert lab[ex["pairs"][0][0]] == k - 1 if k % 32 else True
    assert any(p == "first" and lab[r] == 0 for r, _, _, _, p, _ in ex["pairs"])
    # the clusters: m centroids within one grid unit of their location
    for m in bc.CLUSTER_M:
        rows = ex["rows"][[kd == "cluster %d location" % m for kd in ex["kinds"]]]
        near = np.flatnonzero(np.abs(C - X[rows[0]]).max(axis=1) <= bc.UNIT)
        assert near.size == m
        assert lab[rows[0]] == ex["winners"][m] == near[np.all(C[near] == X[rows[0]], axis=1)][0]
        far = np.sqrt(ko.sqdist_rows(np.delete(C, near, axis=0), X[rows[0]]))
        assert far.min() > bc.SITE_CLEAR
        lv = ex["levels"][[kd.startswith("cluster %d " % m) for kd in ex["kinds"]]]
        assert set(lv) == {2 if m <= bc.KMAXCAND else 3}
    # no empty cluster but the later copies of exact duplicate centroids
    empty = np.flatnonzero(np.bincount(lab, minlength=k) == 0)
    for j in empty:
        assert np.flatnonzero(np.all(C == C[j], axis=1))[0] < j, j
    assert 1 <= empty.size <= 2 * len(bc.CLUSTER_M)
    # the sequence: every step moves points; the eviction points (L2) in every
    # step, a solo cluster (L1) and the 17-cluster's location (L3) in the swap
    ev = ex["rows"][[kd.startswith("evict ") and kd != "evict support" for kd in ex["kinds"]]]
    solo = ex["rows"][np.array(ex["labels"]) == ex["solos"][0]]
    loc17 = ex["rows"][[kd == "cluster 17 location" for kd in ex["kinds"]]]
    assert ev.size == 4 and solo.size == 4 and loc17.size == 2
    for t in range(1, 4):
        prev, cur = steps[t - 1][1], steps[t][1]
        assert (prev != cur).any()
        assert (prev[ev] != cur[ev]).any(), t
    assert (steps[1][1][solo] != steps[2][1][solo]).all()
    # the points on the 17-cluster's location (L3) move in some delta step: with
    # the swap, or when a mean drifts off the location and a duplicate takes over
    assert any((steps[t - 1][1][loc17] != steps[t][1][loc17]).all() for t in range(1, 4))
    np.testing.assert_array_equal(steps[2][1][solo], ex["winners"][17])


def test_case_without_duplicates_has_no_empty_cluster():
    for d, k in [(40, 1500), (12, 4200), (9, 2300)]:
        X, C, ex = bc.case(d, k, False)
        lab = ko.assign(X, C)
        np.testing.assert_array_equal(lab[ex["rows"]], ex["labels"])
        assert np.bincount(lab, minlength=k).min() >= 1

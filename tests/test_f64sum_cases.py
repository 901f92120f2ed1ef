"""The designed sequences of tests/f64sum_cases.py and its restatement of
f64_walk, on the CPU: the layout fixes the assignment, the model equals
NumPy's sequential sums on every case the GPU tests run, every mutant of the
model breaks a case of the family built for it, and each family really has
the property it exists for (ties inside applied transfers, whole groups
applied composed, exact power-of-two landings at a block end, a group end and
mid-block, members on both sides of 2^-1022).  The same counts on min-max
data in the same layout are printed beside them: the gap the families close."""
import math

import numpy as np
import pytest

import f64prog_model as fm
import f64sum_cases as fc
from oracle import kmeans_oracle as ko

RUN_SHAPES = [(3, 2), (5, 20), (4, 40)]  # the device run's
CASES = [(fam, d, k) for fam in fc.F64_FAMILIES for d, k in fc.SHAPES] + [
    (name, v[1], v[2]) for name, v in fc.F32_CASES.items()] + [
    (fam, d, k) for fam in ("pinned_run", "signs_run") for d, k in RUN_SHAPES] + [
    ("signs_prog", 5, 20)]
PARALLEL = [s for s in fc.SHAPES if s[1] <= 64]  # the shapes f64_walk runs at


def _id(case):
    return "%s-d%d-k%d" % case


def _designed(w):
    return {key: x for key, x in w.items() if key[1] >= 1}


def _line(fam, d, k):
    w = _designed(fc.walks(fam, d, k))
    ties = [x.ties for x in w.values()]
    grp = [x.groups for x in w.values()]
    tot = fc.walks(fam, d, k)
    return ("%-13s d=%2d k=%2d: ties per sequence min %d median %d, whole groups min %d max %d, "
            "blocks by transfer %d, walked %d of %d pairs" % (
                fam, d, k, min(ties), int(np.median(ties)), min(grp), max(grp),
                sum(x.blocks for x in tot.values()), sum(x.walked for x in tot.values()),
                fc.pairs(fam, d, k)))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_layout_fixes_assignment_and_model_equals_numpy(case):
    fam, d, k = case
    c = fc.case(*case)
    X, C, lab = c["X"], c["C"], c["labels"]
    assert X.shape == (fc.F32_CASES[fam][0] if fam in fc.F32_CASES
                       else fc.N_OF[fc.VARIANT_OF.get(fam, fam)], d)
    assert X.shape[0] <= 6 * 16384 + 300
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(ko.assign(X, C), lab)
    if fam not in ("large", "large_inf"):
        assert np.bincount(lab, minlength=k).min() > 0
        np.testing.assert_array_equal(X[:, 0], C[lab, 0])
    got = np.zeros(c["sums"].shape)
    for (j, f), x in fc.walks(*case).items():
        got[j, f] = x.sum
    np.testing.assert_array_equal(got, c["sums"])
    np.testing.assert_array_equal(np.signbit(got), np.signbit(c["sums"]))
    print("\n" + _line(*case))


@pytest.mark.parametrize("mutant", sorted(fc.MUTANTS))
def test_every_mutant_breaks_its_family(mutant):
    fam = fc.MUTANTS[mutant]
    broken = {}
    for d, k in PARALLEL[:2]:
        want = fc.case(fam, d, k)["sums"]
        w = fc.walks(fam, d, k, mutant)
        broken[(d, k)] = sum(x.sum != want[j, f] for (j, f), x in w.items())
    print("\nmutant %s on %s: sequences with a wrong sum %s" % (mutant, fam, broken))
    assert any(broken.values()), broken
    # ... and min-max data in the same layout does not notice the parity mutants
    if mutant in ("entry", "exit", "tie_up"):
        want = fc.case("minmax", 3, 2)["sums"]
        w = fc.walks("minmax", 3, 2, mutant)
        print("  on minmax d=3 k=2: %d of %d sequences wrong" % (
            sum(x.sum != want[j, f] for (j, f), x in w.items()), len(w)))


def test_transfers_equal_the_program_model():
    """The vectorised integer transfers of f64sum_cases against
    f64prog_model.block_transfer (real fp64 additions from both entries)."""
    for fam in ("pinned_ties", "growing_ties", "landings"):
        c = fc.case(fam, 5, 20)
        sq = fc._Seq(c["X"][:, 2], c["labels"], 3, fc.F64, None)
        s, seen = float(sq.block(sq.live[0]).sum()), 0
        for li in range(1, len(sq.live), 7):
            s = float(sq.vals[:sq.start[sq.live[li]]].sum())
            e = fm.binade(s)
            want = fm.block_transfer(sq.block(sq.live[li]).tolist(), e)
            got = sq.xfer(li, e)
            if want is None:  # (leaves the binade from its bottom: never applied)
                continue
            assert got is not None and got[:3] == want, (fam, li, got, want)
            seen += 1
        assert seen >= 20


@pytest.mark.parametrize("d,k", fc.SHAPES)
def test_pinned_and_growing_have_ties_in_composed_transfers(d, k):
    for fam in ("pinned_ties", "growing_ties"):
        w = _designed(fc.walks(fam, d, k))
        assert len(w) == k * (d - 1)
        assert min(x.ties for x in w.values()) >= 100, _line(fam, d, k)
        if fam == "pinned_ties":
            # two or more whole groups composed; only the first member's block walked
            assert min(x.groups for x in w.values()) >= 2, _line(fam, d, k)
            assert {x.walked for x in w.values()} == {1}
        print("\n" + _line(fam, d, k))
        print(_line("minmax_small" if fam == "pinned_ties" else "minmax", d, k))
    if (d, k) == (3, 2):  # the largest sequences: binades 0..14
        assert {fm.binade(v) for v in fc.case("growing_ties", d, k)["sums"][:, 1:].ravel()} == {14}


@pytest.mark.parametrize("fam", ["pinned_run", "signs_run"])
@pytest.mark.parametrize("d,k", RUN_SHAPES)
def test_run_variants_keep_every_label(fam, d, k):
    """The designed values of the base family, and three Lloyd steps of the
    oracle that move no row (with the base family's selector the pin rows
    move in the second step)."""
    c, base = fc.case(fam, d, k), fc.case(fc.VARIANT_OF[fam], d, k)
    np.testing.assert_array_equal(c["X"][:, 1:], base["X"][:, 1:])
    np.testing.assert_array_equal(c["labels"], base["labels"])
    X, C = c["X"], c["C"]
    for _ in range(3):
        lab = ko.assign(X, C)
        np.testing.assert_array_equal(lab, c["labels"])
        C = fc.numpy_sums(X, lab, k) / np.bincount(lab, minlength=k)[:, None]
    cnt = np.bincount(base["labels"], minlength=k)
    moved = ko.assign(base["X"], base["sums"] / cnt[:, None]) != base["labels"]
    assert moved.any() or k == 2


def test_signs_prog_fits_the_sharded_programs():
    """signs without its always-negative sequence: every later shard's
    program (f64prog_model.shard_program) stays within the 127 items."""
    c = fc.case("signs_prog", 5, 20)
    X, lab = c["X"], c["labels"]
    n = X.shape[0]
    assert (np.add.accumulate(X[lab == 0, 3]) > 0).all()  # sequence 2 is positive here
    assert (X[:, 1:] < 0).any() and np.signbit(X[:, 1:][X[:, 1:] == 0]).any()
    most = 0
    for W in (2, 3):
        cut = [0] + [r * n // W + 37 * r for r in range(1, W)] + [n]
        for r in range(1, W):
            for j in range(20):
                for f in range(5):
                    off = float(X[:cut[r], f][lab[:cut[r]] == j].sum())
                    items = fm.shard_program(X[cut[r]:cut[r + 1], f], lab[cut[r]:cut[r + 1]],
                                             j, off, 127)
                    assert items is not None, (W, r, j, f)
                    most = max(most, len(items))
    print("\nsigns_prog: at most %d items in a program" % most)


@pytest.mark.parametrize("fam", ["large", "large_sel", "large_inf"])
@pytest.mark.parametrize("d,k", fc.SHAPES)
def test_large_family(fam, d, k):
    c = fc.case(fam, d, k)
    w = _designed(fc.walks(fam, d, k))
    if fam == "large_inf":
        assert np.isinf(c["sums"][0, 1:]).all() and (c["sums"][0, 1:] > 0).all()
        return
    assert np.isfinite(c["sums"]).all()
    assert min(fm.binade(x.sum) for x in w.values()) >= 500
    assert min(x.groups for x in w.values()) >= 2
    if fam == "large_sel":
        assert {x.walked for x in w.values()} == {1}
        assert min(x.ties for x in w.values()) >= 50


@pytest.mark.parametrize("d,k", fc.SHAPES)
def test_landings_hit_the_power_of_two_at_the_three_positions(d, k):
    c = fc.case("landings", d, k)
    X, lab = c["X"], c["labels"]
    seen = set()
    for j in range(k):
        rows = np.flatnonzero(lab == j)
        for f in range(1, d):
            ex = fc.landing_exponent(f)
            m = 2 ** ex
            if rows.size <= m:
                continue
            col = X[rows, f]
            assert (col[:m] == 1.0).all()
            # the running value lands exactly on 2^ex ...
            assert float(np.add.accumulate(col[:m])[-1]) == 2.0 ** ex
            # ... and every addend after it is odd on the old binade's grid
            steps = np.ldexp(col[m:], 53 - ex)
            assert (steps == np.floor(steps)).all() and (steps % 2 == 1).all()
            here, nxt = rows[m - 1] // fc.KFB, rows[m] // fc.KFB
            seen.add("mid-block" if nxt == here else
                     "block end" if nxt // fc.GROUP == here // fc.GROUP else "group end")
            if j == 0:
                assert (here, nxt) == (m // 16 - 1, m // 16)
    assert seen == {"mid-block", "block end", "group end"}, seen
    print("\n" + _line("landings", d, k))
    print(_line("minmax", d, k))  # (landings' n)


@pytest.mark.parametrize("d,k", fc.SHAPES)
def test_tiny_has_members_on_both_sides_of_the_smallest_normal(d, k):
    c = fc.case("tiny", d, k)
    V = c["X"][:, 1:]
    assert V.min() >= 2.0 ** -1074 and V.max() < 2.0 ** -1018
    assert (V < 2.0 ** -1022).any(axis=0).all() and (V >= 2.0 ** -1022).any(axis=0).all()
    w = _designed(fc.walks("tiny", d, k))
    for (j, f), x in w.items():
        assert x.sum > 2.0 ** -1022      # ends in a normal binade ...
        assert x.walked >= 2             # ... after more than one block below it
    print("\n" + _line("tiny", d, k))


@pytest.mark.parametrize("d,k", fc.SHAPES)
def test_signs_sequences(d, k):
    c = fc.case("signs", d, k)
    X, lab, sums = c["X"], c["labels"], c["sums"]
    seq = lambda t: X[lab == t // (d - 1), 1 + t % (d - 1)]
    run = np.add.accumulate(seq(0))
    z = int(np.flatnonzero(run == 0.0)[0])
    assert not np.signbit(run[z]) and z >= 100 and run[-1] > 0.0   # exactly +0.0, then on
    assert np.signbit(seq(1)[:5]).all() and (seq(1)[:5] == 0.0).all()
    assert (np.add.accumulate(seq(2)) < 0.0).all()
    for t in range(3, k * (d - 1)):
        v = seq(t)
        assert 1 <= (v < 0).sum() <= v.size // 1000 + 1
        run = np.add.accumulate(v)
        dip = int(np.flatnonzero(run < 2.0 ** 20)[0])                # dips below the pin, returns
        assert (run[dip:] >= 2.0 ** 20).any()
    w = _designed(fc.walks("signs", d, k))
    assert min(x.walked for x in w.values()) >= 1
    print("\n" + _line("signs", d, k))


@pytest.mark.parametrize("fam", ["growing_ties", "landings"])
@pytest.mark.parametrize("d,k", PARALLEL)
def test_model_walks_under_half_the_device_bound(fam, d, k):
    """The GPU tests bound ctx.f64_walked() by 5 % of the (block, sequence)
    pairs; the model (one walked block per crossing) stays under half of it,
    the selector column included."""
    walked = sum(x.walked for x in fc.walks(fam, d, k).values())
    assert walked < 0.025 * fc.pairs(fam, d, k), _line(fam, d, k)


@pytest.mark.parametrize("name", sorted(fc.F32_CASES))
def test_f32_cases(name):
    n, d, k, mode = fc.F32_CASES[name]
    c = fc.case(name, d, k)
    X = c["X"]
    assert X.dtype == np.float32 and c["sums"].dtype == np.float32
    # the storage gate (decide_mode): F32X needs |x| 2^S < 2^30 on the data's grid 2^-S
    S = 14 if name.endswith("_x") else 16
    assert (np.ldexp(X.astype(np.float64), S) % 1 == 0).all()
    assert (np.ldexp(X.astype(np.float64), S - 1) % 1 != 0).any()
    assert (math.ldexp(float(np.abs(X).max()), S) < 2.0 ** 30) == (mode == 1)
    w = _designed(fc.walks(name, d, k))
    assert min(x.ties for x in w.values()) >= 100, _line(name, d, k)
    if "pinned" in name:
        assert min(x.groups for x in w.values()) >= 2
        assert {x.walked for x in w.values()} == {1}
    else:
        assert sum(x.walked for x in fc.walks(name, d, k).values()) < 0.025 * fc.pairs(name, d, k)
    # the float64 sum of the same values differs: the 24-bit arithmetic is what is tested
    assert (np.add.reduce(X[c["labels"] == 0].astype(np.float64), axis=0)[1:]
            != c["sums"][0, 1:]).any()

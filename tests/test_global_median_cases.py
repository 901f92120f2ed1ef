"""tests/global_median_cases.py builds what it claims (CPU): every expected
median equals the sorted-value contract of csrc/medians.hip,
((0.0 + s[(n-1)//2]) + s[n//2]) / 2 (or (0.0 + s[n//2]) / 1), bit for bit and
never -0.0; the tables have the storage mode, the value range and the planted
middles the GPU tests rely on."""
import numpy as np
import pytest

import global_median_cases as gc


def _same(a, b):
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.signbit(a), np.signbit(b))


@pytest.mark.parametrize("name", gc.CASES)
def test_expected_is_the_sorted_value_contract(name):
    X, exp = gc.case(name)
    _same(exp, gc.sort_medians(X))
    assert not np.signbit(exp).any() or (exp[np.signbit(exp)] != 0).all()
    assert np.isfinite(X).all()
    if name != "minmax":
        assert gc.is_f32x(X) == name.endswith("f32x"), name


def test_row_cases_lie_in_one_binade_and_cover_the_turns():
    for n in gc.ROW_N:
        for m in gc.MODES:
            X, exp = gc.case("rows-%d-%s" % (n, m))
            assert X.shape == (n, 3) and X.min() >= 1.0 and X.max() < 2.0
            # one zero row counted with the n real ones lowers some median
            moved = gc.np_medians(np.concatenate([X, np.zeros((1, 3))]))
            assert (moved < exp).any() or n == 1
    assert {gc.GM_ROWS - 1, gc.GM_ROWS, gc.GM_ROWS + 1} <= set(gc.ROW_N)
    assert 8193 in gc.ROW_N and -(-8193 // gc.ROW_PAD) * gc.ROW_PAD == 16384


def test_feature_cases_straddle_every_chunk_boundary():
    d = set(gc.FEAT_D)
    assert {gc.GM_FEAT, gc.GM_FEAT + 1, 4 * gc.GM_FEAT, 4 * gc.GM_FEAT + 1, 8 * gc.GM_FEAT} <= d
    assert {1, 2, 3, 4, 5} <= d  # quad padding of x32; 17 and 65: a chunk of one column


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("n", gc.PART_N)
def test_planted_middles(n, mode):
    X, exp = gc.case("part-%d-%s" % (n, mode))
    notes = gc.part_notes(mode)
    assert X.shape == (n, len(notes))
    assert sum(nt[0].startswith("byte") for nt in notes) == (4 if mode == "f32x" else 8)
    s = np.sort(X, axis=0)
    for f, (note, _, lo, hi) in enumerate(notes):
        if n % 2 == 0:
            assert (s[n // 2 - 1, f], s[n // 2, f]) == (lo, hi), note
            if note == "signed zeros":
                assert np.signbit(s[n // 2 - 1, f]) and not np.signbit(s[n // 2, f])
                assert exp[f] == 0 and not np.signbit(exp[f])
        else:
            assert (s[n // 2 - 1, f], s[n // 2, f], s[n // 2 + 1, f]) == (lo, hi, hi), note
            assert exp[f] == hi
        if note.startswith("byte"):
            p = int(note.split()[1])
            if mode == "f32x":
                k = np.array([lo, hi], dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)
            else:
                k = np.array([lo, hi]).view(np.uint64)
            # positive values: the order-preserving key is the bits with the top bit set
            diff = int(k[0] ^ k[1])
            assert diff >> (8 * (8 - p)) == 0 and (diff >> (8 * (7 - p))) & 0xFF, (note, hex(diff))


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("n", gc.DEGEN_N)
def test_degenerate_columns(n, mode):
    X, exp = gc.case("degen-%d-%s" % (n, mode))
    assert len(gc.DEGEN_NOTES) == X.shape[1] == 8
    assert np.unique(X[:, 0]).size == 1 and np.unique(X[:, 5]).size == 1
    v, c = np.unique(X[:, 1], return_counts=True)
    assert v.size == 2 and abs(int(c[0]) - int(c[1])) <= 1
    v, c = np.unique(X[:, 2], return_counts=True)
    assert v.size == 2 and sorted(c) == [1, n - 1]
    assert (X[:, 3] == 0.5).sum() == n // 2 + 1 and np.unique(X[:, 3]).size > n // 4
    for f in (4, 6, 7):
        assert np.unique(X[:, f]).size > n // 2


def test_shard_cases():
    for mode in gc.MODES:
        parts, exp = gc.shard_case("three", mode)
        assert [p.shape[0] for p in parts] == [5912, 319, 5]
        parts, exp = gc.shard_case("parity", mode)
        n = sum(p.shape[0] for p in parts)
        assert all(p.shape[0] % 2 != n % 2 for p in parts)
        parts, exp = gc.shard_case("empty", mode)
        assert parts[1].shape == (0, 3)
        _same(exp, gc.sort_medians(np.concatenate(parts)))
        parts, exp = gc.split_middle_case(mode)
        assert (parts[0].max(axis=0) < parts[1].min(axis=0)).all()
        both = np.concatenate(parts)
        _same(exp, gc.sort_medians(both))
        _same(exp, (parts[0].max(axis=0) + parts[1].min(axis=0)) / 2.0)
        for p in parts:
            assert gc.is_f32x(p) == (mode == "f32x")

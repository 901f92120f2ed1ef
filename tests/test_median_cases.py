"""The median case builder (tests/median_cases.py) does what the GPU tests
rely on: the oracle's nearest-centroid assignment of every case is the
designed labelling, the cluster sizes are the designed ones, and the sorted-
value contract stated at the top of csrc/medians.hip equals np.median on
every case (NaN rows of empty clusters included).  No GPU."""
import numpy as np
import pytest

import median_cases as mc
from oracle import kmeans_oracle as ko


@pytest.mark.parametrize("name", mc.CASES + mc.BUILDER_ONLY)
def test_case_is_as_designed(name):
    X, C, lab, sizes = mc.case(name)
    k = sizes.size
    assert C.shape == (k, X.shape[1]) and X.shape[0] == sizes.sum()
    np.testing.assert_array_equal(np.bincount(lab, minlength=k), sizes)
    np.testing.assert_array_equal(ko.assign(X, C), lab)
    f32_exact = np.array_equal(X.astype(np.float32).astype(np.float64), X)
    assert f32_exact == name.endswith("f32x")
    if f32_exact:   # the F32X gate of decide_mode: |x| 2^S < 2^30 on the data's grid
        S = next(s for s in range(150) if np.array_equal(np.ldexp(X, s), np.rint(np.ldexp(X, s))))
        assert np.abs(X).max() * 2.0 ** S < 2.0 ** 30, S
    exp = mc.ref_medians(X, lab, k)
    got = mc.sort_medians(X, lab, k)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))
    np.testing.assert_array_equal(np.isnan(exp[:, 0]), sizes == 0)


def test_sizes_reach_what_they_name():
    # scan ranges: the three largest block cases need a second range
    nr = [-(-(-(-n // mc.MG_BLOCK)) // mc.MG_RANGE) for n in mc.BLOCK_N]
    assert nr == [1, 1, 1, 1, 2, 3]
    assert [-(-n // mc.MG_BLOCK) for n in mc.BLOCK_N] == [1, 1, 2, 64, 65, 130]
    # lane mapping: both loop boundaries of every d
    assert [mc.hist_rows(d) for d in mc.LANE_D] == [1024, 512, 256, 128, 16, 16, 16, 16]
    assert max(max(mc.lane_sizes(d)) for d in mc.LANE_D) == 8193
    for k, d in mc.BIG_K:
        sizes = mc.case("bigk-%d-%d-f32x" % (k, d))[3]
        assert sizes.min() >= 1 and k <= mc.MG_MAXK


@pytest.mark.parametrize("mode", mc.MODES)
def test_planted_columns_have_their_middles(mode):
    """Every planted column's two middle values are the planted ones, and the
    byte columns part at the byte they name (order-preserving keys as in
    medians.hip: 4 bytes for F32X, 8 for F64)."""
    X, C, lab, sizes = mc.case("part-" + mode)
    nbytes = 4 if mode == "f32x" else 8

    def key(v):
        if nbytes == 4:
            b = np.array([v], dtype=np.float32).view(np.uint32)[0]
            return int(~b & 0xFFFFFFFF) if b >> 31 else int(b | 0x80000000)
        b = int(np.array([v], dtype=np.float64).view(np.uint64)[0])
        return (~b & (2 ** 64 - 1)) if b >> 63 else (b | 1 << 63)

    seen = set()
    for j, f, vals, note in mc.part_plants(mode, 11):
        s = np.sort(X[lab == j, f])
        np.testing.assert_array_equal(s, np.sort(vals))
        m = s.size
        a, b = s[(m - 1) // 2], s[m // 2]
        ka, kb = key(a), key(b)
        first = next((p for p in range(nbytes)
                      if (ka >> 8 * (nbytes - 1 - p)) & 0xFF != (kb >> 8 * (nbytes - 1 - p)) & 0xFF),
                     None)
        if note.startswith("byte"):
            assert first == int(note.split()[1]), (note, a, b)
            seen.add(first)
        elif note in ("equal", "ties", "ties, odd"):
            assert a == b and first is None, (note, a, b)
            if note != "equal":   # the run reaches past both middle ranks
                assert s[(m - 1) // 2 - 1] == a == s[m // 2 + 1]
        elif note == "opposite sign":
            assert a < 0 < b and first == 0
        elif note == "neighbours":
            assert first == nbytes - 1 and kb == ka + 1
        elif note == "zeros":
            assert not s.any() and np.signbit(s).any() and not np.signbit(s).all()
        else:
            assert note == "signed zeros in the middle" and a == 0 and b == 0
    assert seen == set(range(nbytes))

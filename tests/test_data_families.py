"""The data families of tests/data_families.py have the properties the GPU
parity cases (test_gpu_data_ranges.py) rely on, for every (family, shape)
those cases use: fp32 exactness, the F32X gate's bounds, k distinct seeds and
no empty cluster in the oracle's Lloyd steps (so that no parity check depends
on the order of np.random reseeds)."""
import numpy as np
import pytest

import data_families as df
from oracle import kmeans_oracle as ko


@pytest.mark.parametrize("case", df.CASES, ids=df.case_id)
def test_family_properties(case):
    name, n, d, k = case
    X = df.data(case)
    assert X.shape == (n, d) and X.dtype == np.float64 and np.isfinite(X).all()
    exact32 = np.array_equal(X.astype(np.float32).astype(np.float64), X)
    assert exact32 == (name in df.F32_EXACT)
    want = df.EXPECT[name]
    if want is not None and want[0] == df.MODE_F32X:
        S = want[1]
        q = np.ldexp(X, S)
        assert np.array_equal(q, np.rint(q))  # on the 2^-S grid ...
        assert S == 0 or (np.ldexp(X, S - 1) % 1.0 != 0).any()  # ... and on no coarser one
        absmax = np.abs(q).max()
        assert absmax < 2.0 ** 30
        assert absmax * n < 2.0 ** 53
        # pre_ok: |x - mu| below 2^24 grid steps (mu = the midrange on the grid)
        mu = np.rint(np.ldexp(np.float32(0.5 * (X.min(axis=0) + X.max(axis=0))).astype(np.float64), S))
        dev = np.maximum(q.max(axis=0) - mu, mu - q.min(axis=0)).max()
        assert (dev < 2.0 ** 24) == want[2], dev
    if name == "int_signed":
        assert X.min() < 0
    if name == "raw_f64":
        assert (X[:, 1::2].min(axis=0) < 0).all() and (X[:, 1::2].max(axis=0) > 0).all()
    ref = df.reference(case)
    assert np.unique(ref["C0"], axis=0).shape[0] == k
    for lab in ref["labels"]:
        assert np.bincount(lab, minlength=k).min() > 0


def test_reference_is_the_oracle_loop():
    """df.reference keeps every step's labels; its result is ko.lloyd's."""
    case = ("int_signed", 16_500, 5, 7)
    ref = df.reference(case)
    C, lab, _, steps = ko.lloyd(df.data(case), ref["C0"], df.loop_steps(7), -1.0)
    assert steps == len(ref["labels"]) == 4
    np.testing.assert_array_equal(C, ref["C"])
    np.testing.assert_array_equal(lab, ref["labels"][-1])


def test_case_list():
    assert len(df.CASES) == 27 == len(set(df.CASES))
    assert all(n > 8192 and n % 8192 for _, n, _, _ in df.CASES)

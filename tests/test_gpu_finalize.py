"""K6 (fin_reduce / fin_apply of csrc/features.hip) at its edges against
oracle/features_oracle.finalize, bit for bit: a single row, constant columns
(max == min -> 0.0), no writes (mean -> 1.0), no accesses (locality -> 1.0),
every creation time null, negative ages, ages one ulp apart, counts around
2^53 and more rows than one launch has threads.  Every case also goes through
features_finalize_stats + features_finalize_apply as two ranks would run them:
the table split into two unequal parts, the statistics merged, n_rows_total
the whole.  tests/event_cases.py builds the tables."""
import numpy as np
import pytest

import event_cases as ec
from oracle import features_oracle as fo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ec.FIN_CASES)
def test_finalize_edges(ctx, name):
    c, cr, obs = ec.fin_case(name)
    n = c.shape[0]
    exp = fo.finalize(c, cr, obs)
    np.testing.assert_array_equal(ctx.features_finalize(c, cr, obs), exp)
    # two ranks: rows [0, cut) and [cut, n)
    cut = n // 3 if n > 1 else 1
    parts = [(c[:cut], cr[:cut]), (c[cut:], cr[cut:])]
    st = [ctx.features_finalize_stats(pc, pcr, obs) for pc, pcr in parts]
    ist = np.array([st[0][0][0] + st[1][0][0]]
                   + [f(st[0][0][i], st[1][0][i]) for i, f in zip(range(1, 7), [min, max] * 3)],
                   dtype=np.int64)
    dst = np.array([f(st[0][1][i], st[1][1][i]) for i, f in zip(range(4), [min, max] * 2)])
    got = np.concatenate([ctx.features_finalize_apply(pc, pcr, obs, ist, dst, n)
                          for pc, pcr in parts])
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))

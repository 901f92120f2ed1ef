"""The host definitions of cluster_agreement.py and replication_plan's
transition arithmetic (CPU): the contingency table against a double loop, the
adjusted Rand index against an independent Fraction evaluation and
scikit-learn, the matching against scipy, the moves against a per-file loop."""
from fractions import Fraction
from math import comb

import numpy as np
import pytest


def loop_table(a, b, ka, kb, sizes=None):
    counts = [[0] * kb for _ in range(ka)]
    nbytes = [[0] * kb for _ in range(ka)]
    for r in range(len(a)):
        counts[int(a[r])][int(b[r])] += 1
        if sizes is not None:
            nbytes[int(a[r])][int(b[r])] += int(sizes[r])
    return counts, nbytes


@pytest.mark.parametrize("n,ka,kb", [(0, 1, 1), (1, 1, 1), (7, 2, 3), (200, 5, 4), (200, 1, 9),
                                     (64, 9, 1)])
def test_contingency_host_against_a_double_loop(n, ka, kb):
    from cluster_agreement import contingency_host

    rng = np.random.default_rng(n + ka)
    a, b = rng.integers(0, ka, n), rng.integers(0, kb, n)
    edge = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62, 2 ** 63 - 1], dtype=np.int64)
    sizes = edge[rng.integers(0, len(edge), n)]
    want_c, want_b = loop_table(a, b, ka, kb, sizes)
    counts = contingency_host(a, b, ka, kb)
    assert counts.dtype == np.int64 and counts.shape == (ka, kb) and counts.tolist() == want_c
    counts2, nbytes = contingency_host(a, b, ka, kb, sizes)
    assert counts2.tolist() == want_c and nbytes.tolist() == want_b
    assert all(type(v) is int for v in nbytes.ravel())


def test_contingency_host_sums_pass_uint64():
    from cluster_agreement import contingency_host

    _, nbytes = contingency_host([0] * 8, [0] * 8, 1, 2, [2 ** 62] * 8)
    assert nbytes.tolist() == [[8 * 2 ** 62, 0]] and 8 * 2 ** 62 > 2 ** 64


def test_contingency_host_refuses_bad_input():
    from cluster_agreement import contingency_host

    for a, b, ka, kb, s in (([0, 2], [0, 0], 2, 1, None), ([0, -1], [0, 0], 2, 1, None),
                            ([0, 1], [0, 1], 2, 1, None), ([0, 1], [0], 2, 1, None),
                            ([0, 1], [0, 0], 2, 1, [1, -1]), ([0, 1], [0, 0], 2, 1, [1]),
                            ([0], [0], 0, 1, None)):
        with pytest.raises(ValueError):
            contingency_host(a, b, ka, kb, s)


def fraction_ari(table):
    """The textbook form (index - expected) / (max - expected), in Fractions."""
    t = [[int(v) for v in row] for row in table]
    n = sum(map(sum, t))
    s = sum(comb(v, 2) for row in t for v in row)
    a = sum(comb(sum(row), 2) for row in t)
    b = sum(comb(sum(col), 2) for col in zip(*t))
    big = comb(n, 2)
    if big == 0:
        return 1.0
    expected = Fraction(a * b, big)
    den = Fraction(a + b, 2) - expected
    return 1.0 if den == 0 else float((s - expected) / den)


def ari_cases():
    rng = np.random.default_rng(7)
    out = [("n2_same", [0, 1], [1, 0]), ("n2_split", [0, 1], [0, 0]), ("n2_one", [0, 0], [0, 0]),
           ("one_cluster", [0] * 50, [0] * 50), ("singletons", list(range(40)), list(range(40))[::-1]),
           ("one_vs_singletons", [0] * 30, list(range(30)))]
    for n, ka, kb, flip in ((10, 2, 3, None), (1000, 4, 4, 0.0), (1000, 4, 4, 0.05), (5000, 64, 64, 0.2),
                            (20000, 64, 64, None), (20000, 3, 1024, None), (2000000, 8, 8, 0.01),
                            (2000000, 64, 64, None)):
        a = rng.integers(0, ka, n)
        if flip is None:
            b = rng.integers(0, kb, n)
        else:
            b = rng.permutation(kb)[a % kb]
            move = rng.random(n) < flip
            b[move] = rng.integers(0, kb, int(move.sum()))
        out.append((f"n{n}_{ka}x{kb}_{flip}", a, b))
    return out


ARI_CASES = ari_cases()


@pytest.mark.parametrize("case", ARI_CASES, ids=[c[0] for c in ARI_CASES])
def test_adjusted_rand_against_fractions_and_sklearn(case):
    from cluster_agreement import adjusted_rand, contingency_host

    _, a, b = case
    a, b = np.asarray(a), np.asarray(b)
    table = contingency_host(a, b, int(a.max()) + 1, int(b.max()) + 1)
    got = adjusted_rand(table)
    assert isinstance(got, float) and got == fraction_ari(table.tolist())
    assert got == adjusted_rand(table.T)
    metrics = pytest.importorskip("sklearn.metrics")
    ref = float(metrics.adjusted_rand_score(a, b))
    # scikit-learn evaluates 2.0 * x / y in floats with at most three roundings, ours has one
    assert abs(got - ref) <= 4 * 2.0 ** -53 * abs(got), (got, ref)


def test_adjusted_rand_degenerate_and_known_values():
    from cluster_agreement import adjusted_rand

    assert adjusted_rand([[0]]) == 1.0 and adjusted_rand([[1]]) == 1.0  # n = 0, n = 1
    assert adjusted_rand([[2]]) == 1.0 and adjusted_rand(np.eye(5, dtype=np.int64)) == 1.0
    assert adjusted_rand([[1, 1]]) == 0.0
    assert adjusted_rand([[5, 0], [0, 5]]) == 1.0 and adjusted_rand([[0, 5], [5, 0]]) == 1.0
    # n = 2^31 - 1 in one cell and split in two: the int64 sums and the products in Python ints
    n = 2 ** 31 - 1
    assert adjusted_rand([[n]]) == 1.0
    assert adjusted_rand([[n // 2, 0], [0, n - n // 2]]) == 1.0
    assert adjusted_rand([[n // 2, n - n // 2]]) == 0.0
    with pytest.raises(ValueError):
        adjusted_rand([[2 ** 31]])
    with pytest.raises(ValueError):
        adjusted_rand([1, 2])


def test_match_clusters_permuted_identity_rectangular_and_ties():
    from scipy.optimize import linear_sum_assignment

    from cluster_agreement import match_clusters

    perm = np.random.default_rng(3).permutation(9)
    table = np.zeros((9, 9), dtype=np.int64)
    table[perm, np.arange(9)] = np.arange(9) + 5  # b-cluster j is a-cluster perm[j]
    table += 1
    assert match_clusters(table).tolist() == perm.tolist()
    wide = np.array([[9, 1, 0, 2], [0, 1, 8, 2]])  # 2 a-clusters, 4 b-clusters
    assert match_clusters(wide).tolist() == [0, -1, 1, -1]
    tall = wide.T  # 4 a-clusters, 2 b-clusters: every b-cluster is matched
    assert match_clusters(tall).tolist() == [0, 2]
    ties = np.ones((4, 4), dtype=np.int64)
    rows, cols = linear_sum_assignment(ties, maximize=True)
    want = np.full(4, -1)
    want[cols] = rows
    assert match_clusters(ties).tolist() == want.tolist()
    with pytest.raises(ValueError):
        match_clusters([1, 2])


def test_transition_from_table_against_a_per_file_loop():
    from cluster_agreement import contingency_host
    from replication_plan import transition_from_table

    rng = np.random.default_rng(11)
    n = 500
    prev_cats, prev_facs = ["Hot", "Cold", "Hot", "(new)"], [3, 1, 3, 2]
    cats, facs = ["Cold", "Hot", "Warm"], [1, 3, 2]
    old = rng.integers(0, 4, n)
    new = rng.integers(0, 3, n)
    sizes = rng.integers(0, 2 ** 40, n).astype(np.int64)
    sizes[:4] = [2 ** 62, 2 ** 62, 2 ** 32, 0]
    old[:2], new[:2] = 1, 1  # factor 1 -> 3 on 2^63 bytes: the copy passes int64
    want = {}
    total = dict(files=0, bytes=0, bytes_to_copy=0, bytes_to_free=0, files_changed=0)
    for o, w, s in zip(old.tolist(), new.tolist(), sizes.tolist()):
        fo, fn = prev_facs[o], facs[w]
        row = want.setdefault(prev_cats[o], {}).setdefault(
            cats[w], dict(old_factor=fo, new_factor=fn, files=0, bytes=0, bytes_to_copy=0,
                          bytes_to_free=0))
        add = dict(files=1, bytes=s, bytes_to_copy=max(fn - fo, 0) * s, bytes_to_free=max(fo - fn, 0) * s)
        for key, v in add.items():
            row[key] += v
            total[key] += v
        total["files_changed"] += fo != fn
    counts, nbytes = contingency_host(old, new, 4, 3, sizes)
    got = transition_from_table(counts, nbytes, prev_cats, prev_facs, cats, facs)
    assert got == {"moves": want, "total": total}
    assert got["total"]["bytes_to_copy"] > 2 ** 63
    moves = got["moves"]
    assert moves["Cold"]["Hot"]["bytes_to_free"] == 0 and moves["Cold"]["Hot"]["bytes_to_copy"] > 0  # up
    assert moves["Hot"]["Cold"]["bytes_to_copy"] == 0 and moves["Hot"]["Cold"]["bytes_to_free"] > 0  # down
    assert moves["Hot"]["Hot"]["bytes_to_copy"] == moves["Hot"]["Hot"]["bytes_to_free"] == 0
    assert moves["(new)"]["Warm"]["bytes_to_copy"] == moves["(new)"]["Warm"]["bytes_to_free"] == 0
    assert moves["(new)"]["Hot"]["old_factor"] == 2
    # without sizes: files only
    plain = transition_from_table(counts, None, prev_cats, prev_facs, cats, facs)
    assert plain["total"] == {"files": n, "files_changed": total["files_changed"]}
    assert set(plain["moves"]["Hot"]["Cold"]) == {"old_factor", "new_factor", "files"}
    # pairs without files are not listed
    empty = transition_from_table(np.zeros((4, 3), dtype=np.int64), None, prev_cats, prev_facs, cats, facs)
    assert empty == {"moves": {}, "total": {"files": 0, "files_changed": 0}}
    with pytest.raises(ValueError):
        transition_from_table(counts.T, None, prev_cats, prev_facs, cats, facs)
    with pytest.raises(ValueError, match="two pairs of factors"):
        transition_from_table(counts, None, prev_cats, [3, 1, 2, 2], cats, facs)

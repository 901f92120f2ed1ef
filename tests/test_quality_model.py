"""The NumPy model of silhouette and Davies-Bouldin (tests/quality_model.py)
against scikit-learn, live where it is installed and through the fixture
tests/golden/quality_cases.npz everywhere (CPU).

The fixture was recorded with scikit-learn 1.7.2 by `python
tests/test_quality_model.py`: silhouette_samples(D, labels,
metric="precomputed") with D the model's own difference-form distances, and
davies_bouldin_score(X, labels).  Cases: 3 blobs of 300 x 5; a singleton
cluster; an empty cluster id (labels 0, 1, 3).
"""
import os

import numpy as np
import pytest

import quality_model as qm
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "quality_cases.npz")
CASES = ("blobs", "singleton", "empty_id")


def _cases():
    rng = np.random.default_rng(20261019)
    out = {}
    centres = rng.random((3, 5)) * 4.0
    out["blobs"] = (np.concatenate([c + 0.3 * rng.standard_normal((300, 5)) for c in centres]),
                    np.repeat(np.arange(3), 300))
    X = rng.random((41, 3))
    lab = np.repeat(np.arange(2), [20, 20]).tolist() + [2]
    X[40] += 3.0
    out["singleton"] = (X, np.array(lab))
    X = np.concatenate([c + 0.2 * rng.standard_normal((30, 4)) for c in rng.random((3, 4)) * 3.0])
    out["empty_id"] = (X, np.repeat(np.array([0, 1, 3]), 30))
    return out


def _sklearn_values(X, labels):
    from sklearn.metrics import davies_bouldin_score, silhouette_samples

    D = qm.distances(X, 0, X.shape[0])
    return silhouette_samples(D, labels, metric="precomputed"), davies_bouldin_score(X, labels)


def _check(X, labels, s_ref, db_ref):
    m, d = X.shape
    k = int(labels.max()) + 1
    s, csum, ccnt = qm.silhouette_samples(X, labels, k)
    np.testing.assert_allclose(s, s_ref, rtol=0, atol=qm.sil_atol(m, d))
    assert np.array_equal(ccnt, np.bincount(labels, minlength=k))
    np.testing.assert_allclose(csum, np.bincount(labels, weights=s_ref, minlength=k), rtol=0,
                               atol=m * qm.sil_atol(m, d))
    C = qm.cluster_means(X, labels, k)
    db = qm.davies_bouldin(X, labels, C)
    # The two sides' centroid means differ by <= m u max|x| per coordinate, which
    # moves any distance to or between centroids by <= shift; on top of that S_j
    # is within scatter_rtol and M_jl within (d/2 + 2) u.  DB is a mean of
    # (S_j + S_l) / M_jl: relative error <= rel_S + rel_M to first order, doubled.
    sums, counts = qm.scatter(X, labels, C)
    ne = np.flatnonzero(counts)
    S = sums[ne] / counts[ne]
    M = np.linalg.norm(C[ne][:, None, :] - C[ne][None, :, :], axis=2)
    shift = 2.0 * np.sqrt(d) * m * qm.U * np.abs(X).max()
    rel_S = qm.scatter_rtol(m, d) + shift / S[S > 0].min()  # (a singleton's S_j is 0 on both sides)
    rel_M = (d / 2.0 + 2.0) * qm.U + shift / M[M > 0].min()
    assert abs(db - db_ref) <= 2.0 * (rel_S + rel_M) * db_ref


@pytest.mark.parametrize("name", CASES)
def test_model_matches_sklearn(name):
    pytest.importorskip("sklearn")
    X, labels = _cases()[name]
    _check(X, labels, *_sklearn_values(X, labels))


@pytest.mark.parametrize("name", CASES)
def test_model_matches_recorded_sklearn(name):
    with np.load(FIXTURE) as z:
        X, labels, s_ref, db_ref = (z[f"{name}_X"], z[f"{name}_labels"], z[f"{name}_s"],
                                    float(z[f"{name}_db"]))
    _check(X, labels, s_ref, db_ref)


def test_model_special_cases():
    X = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [3.0, 4.0], [3.0, 4.5], [9.0, 9.0]])
    labels = np.array([0, 0, 0, 1, 1, 2])
    s, _, _ = qm.silhouette_samples(X, labels)
    assert np.all(s[:3] == 1.0)  # identical points: a_i = 0 exactly
    assert s[5] == 0.0           # singleton
    with pytest.raises(ValueError):
        qm.silhouette_samples(X, np.zeros(6, dtype=np.int64))
    with pytest.raises(ValueError):
        qm.silhouette_samples(X, np.arange(6))


if __name__ == "__main__":
    rec = {}
    for nm, (X_, lab_) in _cases().items():
        s_, db_ = _sklearn_values(X_, lab_)
        rec.update({f"{nm}_X": X_, f"{nm}_labels": lab_, f"{nm}_s": s_, f"{nm}_db": np.float64(db_)})
    np.savez_compressed(FIXTURE, **rec)
    print("wrote", FIXTURE)

"""Cluster validity indices on MI355X: silhouette and Davies-Bouldin.

An extension with no counterpart in the reference, which fixes ``--k 4``
(src/main.py): these two indices are what chooses k.  Inertia
(``ctx.last_inertia``) cannot, it falls with every added cluster.

Both work on what ``kmeans_plusplus.kmeans`` leaves behind in the context: the
resident points and the labels of the last assignment.  The distance is the
reference's own ``np.linalg.norm(x - y)`` (src/kmeans_plusplus.py:33): the
difference form in fp64, on the float64 values of the points.  Every O(m^2) and
O(n) operation runs in libcdr.so (csrc/quality.hip); the host keeps the
sampling, the k x k part of Davies-Bouldin and the sweep's control flow.

Silhouette of m rows (all, or a sample), labels in [0, k), c_A rows labelled A:
    a_i = sum_{j in A, j != i} d(i, j) / (c_A - 1)
    b_i = min over B != A with c_B > 0 of sum_{j in B} d(i, j) / c_B
    s_i = (b_i - a_i) / max(a_i, b_i);  0 when a_i = b_i = 0 or c_A == 1
    score = mean of s_i.  Clusters empty in the sample are skipped.
Davies-Bouldin over all n rows with centroids C:
    S_j = mean over cluster j of d(x, C_j),  M_jl = d(C_j, C_l)
    DB = mean over non-empty j of max_{l != j, non-empty} (S_j + S_l) / M_jl
    (a pair of coincident centroids contributes 0, as scikit-learn has it).

Single context only: there is no sharded form, and a ``comm`` raises
``NotImplementedError``.
"""
from __future__ import annotations

import numpy as np

import kmeans_plusplus as _kp
from _cdr import Context, default_context

__all__ = ["silhouette", "davies_bouldin", "sweep", "stability", "DEFAULT_SAMPLE"]

DEFAULT_SAMPLE = 65536  # rows of the default silhouette sample (4.3e9 pairs)


def _context(X, context, comm) -> Context:
    if comm is not None:
        raise NotImplementedError("cluster_quality: points sharded over a communicator are not "
                                  "supported (single context only)")
    ctx = context if context is not None else default_context()
    if X is not None:
        ctx.load_points(np.asarray(X))
    return ctx


def silhouette(X=None, labels=None, *, k=None, sample_size=None, random_state=None,
               indices=None, context: Context | None = None, comm=None):
    """Silhouette of the resident points (``X=None``) or of X (loaded first).

    labels: one per row (n,), or None for the labels of the last assignment on
    the device.  k: labels are in [0, k); default max(labels) + 1 (pass it for
    a large resident set: the default reads all n labels back).  The rows
    scored are ``indices`` (local rows, any order, no repeats expected), or the
    sample ``np.sort(np.random.default_rng(random_state).choice(n,
    size=sample_size, replace=False))``; sample_size None means all n rows when
    n <= 65536, else 65536.

    Returns ``(score, per_cluster_mean (k,), s (m,), indices (m,))``: s in the
    order of indices, per_cluster_mean NaN for a cluster empty in the sample.
    ValueError when the non-empty clusters of the sample are fewer than 2 or
    more than m - 1 (as scikit-learn), or a label is outside [0, k).
    """
    ctx = _context(X, context, comm)
    n = ctx.info()["n"]
    if labels is not None:
        labels = np.asarray(labels).astype(np.int64, copy=False).ravel()
        if labels.size != n:
            raise ValueError(f"labels has {labels.size} entries for {n} rows")
    if indices is not None:
        if sample_size is not None:
            raise ValueError("pass indices or sample_size, not both")
        indices = np.ascontiguousarray(indices, dtype=np.int64).ravel()
        idx = indices
    else:
        if sample_size is None:
            sample_size = n if n <= DEFAULT_SAMPLE else DEFAULT_SAMPLE
        if sample_size == n:  # the sorted sample of all n rows is every row
            indices, idx = np.arange(n, dtype=np.int64), None
        else:
            indices = np.sort(np.random.default_rng(random_state).choice(
                n, size=int(sample_size), replace=False)).astype(np.int64)
            idx = indices
    if k is None:
        if labels is not None:
            k = int(labels.max()) + 1 if labels.size else 1
        else:
            k = int(ctx.labels().max()) + 1
    sample_labels = None
    if labels is not None:
        if idx is not None and idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError("row index out of range")
        sample_labels = labels if idx is None else labels[idx]
    s, csum, ccnt = ctx.silhouette(k, idx, sample_labels)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_cluster = csum / ccnt.astype(np.float64)
    return float(np.mean(s)), per_cluster, s, indices


def _db_from_scatter(C: np.ndarray, sums: np.ndarray, counts: np.ndarray) -> float:
    ne = np.flatnonzero(counts > 0)
    if ne.size < 2:
        raise ValueError(f"Davies-Bouldin needs at least 2 non-empty clusters, got {ne.size}")
    S = sums[ne] / counts[ne].astype(np.float64)
    Cn = C[ne]
    M = np.linalg.norm(Cn[:, None, :] - Cn[None, :, :], axis=2)
    M[M == 0.0] = np.inf
    R = (S[:, None] + S[None, :]) / M
    np.fill_diagonal(R, 0.0)
    return float(np.mean(R.max(axis=1)))


def davies_bouldin(centroids, X=None, labels=None, *, context: Context | None = None,
                   comm=None) -> float:
    """Davies-Bouldin index of all n resident rows (``X=None``) or of X, with
    the given centroids (k, d) and labels (n,), None = the last assignment's.
    Straight after ``kmeans()`` its returned centroids are the means of its
    returned labels, so this is scikit-learn's ``davies_bouldin_score``.
    ValueError with fewer than 2 non-empty clusters."""
    ctx = _context(X, context, comm)
    C = np.ascontiguousarray(centroids, dtype=np.float64)
    sums, counts = ctx.quality_scatter(C, labels)
    return _db_from_scatter(C, sums, counts)


def sweep(X, ks, *, random_state=None, max_iter=None, sample_size=None,
          context: Context | None = None, comm=None) -> list:
    """``kmeans`` for every k of ks on one load of X, scored.  One dict per k:
    ``k``, ``inertia`` (the device loop's, None when another path ran),
    ``silhouette`` (of the sample of ``silhouette``: the same rows for every
    k), ``davies_bouldin`` and ``nonempty`` clusters.  Host control flow
    only; the indices are NaN for a k that leaves fewer than 2 clusters."""
    X = np.asarray(X)
    ctx = _context(X, context, comm)
    rows = []
    for k in ks:
        k = int(k)
        ctx.last_inertia = None
        centroids, _ = _kp._kmeans_loaded(ctx, X, k, 100, 1e-4, random_state, max_iter)
        sums, counts = ctx.quality_scatter(np.asarray(centroids, dtype=np.float64))
        nonempty = int(np.count_nonzero(counts))
        try:
            sil = silhouette(k=k, sample_size=sample_size, random_state=random_state,
                             context=ctx)[0]
            db = _db_from_scatter(np.asarray(centroids, dtype=np.float64), sums, counts)
        except ValueError:
            sil, db = float("nan"), float("nan")
        rows.append({"k": k, "inertia": ctx.last_inertia, "silhouette": sil,
                     "davies_bouldin": db, "nonempty": nonempty})
    return rows


def stability(X, k, random_states, *, max_iter=None, context: Context | None = None,
              comm=None) -> dict:
    """Whether k gives the same partition from different seeds: ``kmeans`` with
    every seed of random_states (at least 2) on one load of X, and the adjusted
    Rand index of each further run against the first.  The first run's labels
    are kept on the device (``cluster_agreement.keep``) and every comparison is
    one contingency table of the resident against the kept labels
    (``cluster_agreement.contingency``): the comparison moves no label array to
    the host (each ``kmeans`` run itself still returns its labels, as in ``sweep``).
    Returns ``{"k", "ari": [one per further seed], "mean", "min"}``."""
    import cluster_agreement as _ca

    X = np.asarray(X)
    seeds = list(random_states)
    if len(seeds) < 2:
        raise ValueError("stability needs at least 2 random states")
    ctx = _context(X, context, comm)
    k = int(k)
    ari = []
    for j, seed in enumerate(seeds):
        _kp._kmeans_loaded(ctx, X, k, 100, 1e-4, seed, max_iter)
        if j == 0:
            _ca.keep(context=ctx)
        else:
            ari.append(_ca.adjusted_rand(_ca.contingency(ka=k, kb=k, context=ctx)))
    return {"k": k, "ari": ari, "mean": float(np.mean(ari)), "min": float(min(ari))}

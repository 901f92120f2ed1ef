"""NumPy restatement of the two cluster-quality definitions (test helper).

Distances are np.linalg.norm(X[r0:r1, None, :] - X[None, :, :], axis=2): the
reference's difference form (src/kmeans_plusplus.py:33) in fp64, in row chunks
of at most 64 so that d = 64 stays within memory.  Per-cluster sums are
np.add.reduceat over label-sorted columns.
"""
import numpy as np

ROW_CHUNK = 64
U = 2.0 ** -53  # unit roundoff of fp64


def distances(X, r0, r1):
    X = np.asarray(X, dtype=np.float64)
    return np.linalg.norm(X[r0:r1, None, :] - X[None, :, :], axis=2)


def silhouette_samples(X, labels, k=None):
    """(s (m,), per-cluster sum of s (k,), per-cluster counts (k,))."""
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    m = X.shape[0]
    if k is None:
        k = int(labels.max()) + 1
    counts = np.bincount(labels, minlength=k)
    present = np.flatnonzero(counts)
    if not 2 <= present.size <= m - 1:
        raise ValueError("number of non-empty clusters outside [2, m - 1]")
    order = np.argsort(labels, kind="stable")
    starts = np.concatenate(([0], np.cumsum(counts[present])[:-1]))
    seg_of = np.full(k, -1)
    seg_of[present] = np.arange(present.size)
    cnt = counts[present].astype(np.float64)
    s = np.zeros(m)
    for r0 in range(0, m, ROW_CHUNK):
        r1 = min(m, r0 + ROW_CHUNK)
        D = distances(X, r0, r1)[:, order]
        sums = np.add.reduceat(D, starts, axis=1)  # (rows, segments)
        rows = np.arange(r1 - r0)
        own = seg_of[labels[r0:r1]]
        c_own = cnt[own]
        with np.errstate(invalid="ignore", divide="ignore"):
            a = sums[rows, own] / (c_own - 1.0)
            means = sums / cnt[None, :]
            means[rows, own] = np.inf
            b = means.min(axis=1)
            si = (b - a) / np.maximum(a, b)
        si[~np.isfinite(si)] = 0.0  # a = b = 0
        si[c_own == 1.0] = 0.0
        s[r0:r1] = si
    return s, np.bincount(labels, weights=s, minlength=k), counts


def silhouette_score(X, labels, k=None):
    return float(np.mean(silhouette_samples(X, labels, k)[0]))


def scatter(X, labels, C):
    """Per-cluster sums of d(x, C_label) and counts."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    k = C.shape[0]
    dist = np.empty(X.shape[0])
    for r0 in range(0, X.shape[0], 65536):
        r1 = r0 + 65536
        dist[r0:r1] = np.linalg.norm(X[r0:r1] - C[labels[r0:r1]], axis=1)
    return np.bincount(labels, weights=dist, minlength=k), np.bincount(labels, minlength=k)


def davies_bouldin(X, labels, C):
    C = np.asarray(C, dtype=np.float64)
    sums, counts = scatter(X, labels, C)
    ne = np.flatnonzero(counts)
    if ne.size < 2:
        raise ValueError("fewer than 2 non-empty clusters")
    S = sums[ne] / counts[ne]
    M = np.linalg.norm(C[ne][:, None, :] - C[ne][None, :, :], axis=2)
    M[M == 0.0] = np.inf
    R = (S[:, None] + S[None, :]) / M
    np.fill_diagonal(R, 0.0)
    return float(np.mean(R.max(axis=1)))


def cluster_means(X, labels, k):
    X = np.asarray(X, dtype=np.float64)
    C = np.zeros((k, X.shape[1]))
    for j in range(k):
        if np.any(labels == j):
            C[j] = X[labels == j].mean(axis=0)
    return C


def sil_atol(m, d):
    """|s_i| error of two evaluations: each side's a_i, b_i carry a relative
    error <= eps = (m + d/2 + 2) u, so s_i is off by <= 2 eps + 4 u per side."""
    return 4.0 * (m + d / 2.0 + 6.0) * U


def scatter_rtol(n, d):
    return 2.0 * (n + d / 2.0 + 2.0) * U

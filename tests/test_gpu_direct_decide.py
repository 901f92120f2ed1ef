"""screen32bs16's direct test: a re-read point is decided
from its fp32 distances to its centroid and that centroid's two nearest
neighbours, every other centroid bounded through h3; what it leaves undecided
takes the split screen in its batch (kDirectDense or more lanes) or goes to
the wave's tail as a "not screened" record.

Every case runs the device loop for 12-14 steps with tol = -1, one step at a
time so the counters of the bounded steps can be told apart, and asserts
labels and centroids bit-equal to kmeans_oracle.lloyd, with the direct test
(default) and without it (CDR_S32BS_DIRECT=0), the kernel's name, and that the
bounded path ran (tight_points >= n)."""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from oracle import synth

pytestmark = pytest.mark.gpu

FIRST_BOUNDED = 2  # step index: the full screen, the bound rebuild, then screen32bs16


def _grid_uniform(n, d, seed):
    rng = np.random.default_rng(seed)
    return np.floor(rng.random((n, d)) * 2.0 ** 24) * 2.0 ** -24


def _farthest_first(X, k):
    idx = [0]
    dmin = ((X - X[0]) ** 2).sum(axis=1)
    for _ in range(1, k):
        idx.append(int(np.argmax(dmin)))
        dmin = np.minimum(dmin, ((X - X[idx[-1]]) ** 2).sum(axis=1))
    return X[np.array(idx)]


@functools.lru_cache(maxsize=None)
def _split_blobs(n, d, blobs, per):
    """`blobs` separated blobs and `per` start centroids drawn from each: every
    blob is shared by `per` centroids, which keep moving against each other."""
    X = synth.generate(n, 0, n, d, blobs, 17 * n + d)
    F = _farthest_first(X, blobs)  # one point per blob
    b = ((X[:, None, :] - F[None]) ** 2).sum(-1).argmin(1)
    rng = np.random.default_rng(blobs * per + d)
    C0 = np.concatenate([X[np.sort(rng.choice(np.flatnonzero(b == j), per, replace=False))]
                         for j in range(blobs)])
    return _frozen(X, C0)


def _frozen(X, C0):
    for a in (X, C0):
        a.setflags(write=False)
    return X, C0


@functools.lru_cache(maxsize=None)
def _oracle(key, steps):
    X, C0 = _DATA[key]()
    np.random.seed(3)
    C, lab, _, _ = ko.lloyd(X, C0, steps, -1.0)
    for a in (C, lab):
        a.setflags(write=False)
    return C, lab


def _mirror(n, d, k):
    """x and 1 - x (exact on the 2^-24 grid) with mirrored start centroids,
    and points at and a few grid steps around the centre 1/2, equidistant
    from every mirrored centroid pair: exact and near ties every step."""
    h = synth.generate(n // 2, 0, n // 2, d, k // 2, n + d)
    X = np.concatenate([h, 1.0 - h])
    m = n // 50
    rng = np.random.default_rng(n + d)
    X[:m] = 0.5 + np.ldexp(rng.integers(-3, 4, (m, d)).astype(np.float64), -24)
    half = X[m + np.sort(rng.choice(n // 2 - m, k // 2, replace=False))]
    return _frozen(X, np.concatenate([half, 1.0 - half]))


def _few(k):
    n, d = 20_003, 5
    X = synth.generate(n, 0, n, d, 3, 17 * n + d)
    return _frozen(X, X[np.sort(np.random.default_rng(k + d).choice(n, k, replace=False))])


def _uniform(n, d, k):
    X = _grid_uniform(n, d, n + d)
    return _frozen(X, X[np.sort(np.random.default_rng(k + d).choice(n, k, replace=False))])


_DATA = {
    "split16": lambda: _split_blobs(60_001, 16, 8, 3),
    "split8": lambda: _split_blobs(60_001, 8, 8, 3),
    "split3": lambda: _split_blobs(60_001, 3, 8, 3),
    "few2": lambda: _few(2),
    "few3": lambda: _few(3),
    "few4": lambda: _few(4),
    "mirror16": functools.lru_cache(maxsize=None)(lambda: _mirror(40_000, 16, 64)),
    "mirror8": functools.lru_cache(maxsize=None)(lambda: _mirror(30_000, 8, 32)),
    "uniform3": functools.lru_cache(maxsize=None)(lambda: _uniform(90_007, 3, 7)),
}


def _run(ctx, monkeypatch, X, C0, steps, direct=True, split=False, dbg=False, cus=None):
    """`steps` device-loop steps enqueued one at a time: (labels, centroids,
    the profile counters after every step)."""
    from cdr_dist import DeviceLloyd

    monkeypatch.setenv("CDR_BOUNDS", "1")
    monkeypatch.setenv("CDR_S32B_SPLIT", "1")
    monkeypatch.setenv("CDR_S32BS_SPLIT", "1" if split else "0")
    monkeypatch.setenv("CDR_S32BS_DIRECT", "1" if direct else "0")
    monkeypatch.setenv("CDR_BOUNDS_DBG", "1" if dbg else "0")
    if cus is None:
        monkeypatch.delenv("CDR_S32BS_CUS", raising=False)
    else:
        monkeypatch.setenv("CDR_S32BS_CUS", str(cus))
        monkeypatch.setenv("CDR_S32BS_DYN_MIN", "2")
    ctx.load_points(X)
    ctx.profile_reset(True)
    np.random.seed(3)
    run = DeviceLloyd(ctx, np.array(C0, dtype=np.float64), -1.0, lambda g: X[g], X.shape[0])
    prof = []
    try:
        for s in range(steps):
            assert run.advance(1) == 1
            prof.append(ctx.profile_read())
            if s >= FIRST_BOUNDED:
                want = "screen32bs<" if split else "screen32bs16<"
                assert ctx.profile_kernel().startswith(want), ctx.profile_kernel()
        lab, C = ctx.labels(), ctx.lloyd_read()[0]
    finally:
        ctx.lloyd_end()
        ctx.profile_reset(False)
    return lab, C, prof


def _check(ctx, monkeypatch, key, steps, **kw):
    """Both decisions against the oracle; returns the direct run's counters."""
    X, C0 = _DATA[key]()
    C_ref, lab_ref = _oracle(key, steps)
    out = None
    for direct in (True, False):
        lab, C, prof = _run(ctx, monkeypatch, X, C0, steps, direct=direct, **kw)
        np.testing.assert_array_equal(lab, lab_ref, err_msg=f"labels, direct={direct}")
        np.testing.assert_array_equal(C, C_ref, err_msg=f"centroids, direct={direct}")
        print(f"\n{key} direct={direct}: {prof[-1]}")
        assert prof[-1]["tight_points"] >= X.shape[0], prof[-1]
        out = out or prof
    return out


def _after_first(prof, name):
    """Counter `name` over the bounded steps after the first one."""
    return prof[-1][name] - prof[FIRST_BOUNDED][name]


@pytest.mark.parametrize("key", ["split16", "split8", "split3"])
def test_split_blobs_decided_directly(ctx, monkeypatch, key):
    """8 blobs shared by three centroids each (Q = 4, 2, 1): the k-way screen
    decides less than a quarter of the re-read points of the bounded steps
    after the first (an oracle-only model of the rule leaves below 0.1 %
    undecided on these inputs; the triangle test alone sends most of them on),
    so the case fails with the direct test silently off."""
    prof = _check(ctx, monkeypatch, key, 13)
    q, t = _after_first(prof, "queued_points"), _after_first(prof, "tight_points")
    print(f"{key}: queued {q} of {t} re-read")
    assert t > 0 and q < 0.25 * t, (q, t)


def test_split_blobs_four_byte_words(ctx, monkeypatch):
    """The split form (CDR_S32BS_SPLIT=1: screen32bz's lists, no deferral):
    undecided lanes take the in-batch screen."""
    prof = _check(ctx, monkeypatch, "split16", 12, split=True)
    q, t = _after_first(prof, "queued_points"), _after_first(prof, "tight_points")
    assert t > 0 and q < 0.25 * t, (q, t)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_few_centroids(ctx, monkeypatch, k):
    """k = 2 and 3: a neighbour and h3 are absent (+inf); k = 4: both finite
    for the first time."""
    _check(ctx, monkeypatch, f"few{k}", 12)


@pytest.mark.parametrize("key", ["mirror16", "mirror8"])
def test_exact_and_near_ties(ctx, monkeypatch, key):
    """Mirrored data: the points at the centre tie between mirrored centroids;
    the labels are the oracle's lowest-index choice and the tied points reach
    the exact fp64 pass."""
    prof = _check(ctx, monkeypatch, key, 12)
    assert prof[-1]["fallback_points"] > 0, prof[-1]


def test_dense_undecided_batches_and_tail_records(ctx, monkeypatch):
    """Uniform data, every bound failing every step (CDR_BOUNDS_DBG=1): the
    batches' undecided counts lie on both sides of kDirectDense, so in-batch
    screens and "not screened" tail records occur in one launch; then the
    same on an 8-CU grid with the dynamic tail."""
    prof = _check(ctx, monkeypatch, "uniform3", 12, dbg=True)
    n = _DATA["uniform3"]()[0].shape[0]
    assert _after_first(prof, "tight_points") == (12 - 1 - FIRST_BOUNDED) * n, prof[-1]
    assert 0 < _after_first(prof, "queued_points") < _after_first(prof, "tight_points")
    _check(ctx, monkeypatch, "uniform3", 12, dbg=True, cus=8)


def _plan_fields(blk, k):
    rows = blk[: 64 * 20].reshape(64, 20)
    return {"c32": rows[:k, :16].view(np.uint32), "n": rows[:, 16:18].view(np.int32),
            "h3": rows[:, 18].view(np.uint32), "ec32": rows[:, 19].view(np.uint32),
            "E": blk[1280:1344].view(np.uint32), "h": blk[1344:1408].view(np.uint32)}


@pytest.mark.parametrize("k", [2, 3, 4, 7, 40])
def test_plan_builders_agree(ctx, monkeypatch, k):
    """The host plan, plan32_kernel and the finalize build the same prune
    block, bit for bit, for the same centroids: the means of one loop step
    over clusters of coincident points on a coarse grid (every sum exact), with
    centroids 1 and 2 at equal distance from centroid 0 (the lower index is the
    nearer neighbour) and, from k = 4 on, 3 and 4 or "none" following."""
    d = 6
    rng = np.random.default_rng(k)
    P = 0.25 + np.floor(rng.random((k, d)) * 64.0) / 128.0
    P[0] = 0.5
    if k > 2:
        P[1], P[2] = P[0], P[0]
        P[1, 0] += 2.0 ** -5
        P[2, 1] -= 2.0 ** -5
    X = np.repeat(P, 64, axis=0)
    monkeypatch.setenv("CDR_BOUNDS", "1")
    from cdr_dist import DeviceLloyd

    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, P.copy(), -1.0, lambda g: X[g], X.shape[0])
    try:
        assert run.advance(1) == 1
        C = ctx.lloyd_read()[0]
        np.testing.assert_array_equal(C, P)
        fin = _plan_fields(ctx.debug_plan32(2, None, k), k)
        host = _plan_fields(ctx.debug_plan32(0, C, k), k)
        dev = _plan_fields(ctx.debug_plan32(1, C, k), k)
    finally:
        ctx.lloyd_end()
    for name in host:
        np.testing.assert_array_equal(dev[name], host[name], err_msg=f"plan32_kernel: {name}")
        np.testing.assert_array_equal(fin[name], host[name], err_msg=f"finalize: {name}")
    # against NumPy: the two nearest other centroids, ties to the lower index
    D = ((P[:, None, :] - P[None]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")
    for j in range(k):
        want = [int(order[j, i]) if i < k - 1 else -1 for i in range(2)]
        assert host["n"][j].tolist() == want, (j, host["n"][j], want)
    if k > 2:
        assert host["n"][0].tolist() == [1, 2]
    h3 = host["h3"].view(np.float32)
    assert np.all(np.isinf(h3[k:])) and np.all(host["n"][k:] == -1)
    if k <= 3:
        assert np.all(np.isinf(h3[:k]))
    else:
        # h3 / h = third-smallest / smallest pair distance, up to the bounds' slack
        third, first = np.sqrt(np.sort(D, axis=1)[:, 2]), np.sqrt(np.sort(D, axis=1)[:, 0])
        ratio = h3[:k].astype(np.float64) / host["h"].view(np.float32)[:k]
        np.testing.assert_allclose(ratio, third / first, rtol=2.0 ** -18)

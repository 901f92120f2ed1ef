"""The dispatch of the fused F64 assignment (f64_cent_prep<D> and
f64_assign_block<D>, one instantiation per d in 2..16) through its three
callers: the single step (cdr_lloyd_step_f64), the device-resident run
(cdr_lloyd_f64_run: the transfer cache's per-block label-change flags) and the
sharded step (cdr_f64s_begin).  k = 5 takes the fp32 screen, k = 20 (above
the screen's 16 centroids) the exact argmin alone.  n = 10 * 256 + 77 rows are
11 blocks of 256, so the 8-way block renumbering has a quotient and a
remainder and the last block is ragged."""
import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from test_gpu_f64_update import _f64_shards_step, _minmax, _numpy_sums

pytestmark = pytest.mark.gpu

N = 10 * 256 + 77
SPLIT = 1000 + 37
KS = (5, 20)


def _case(d, k):
    rng = np.random.default_rng(1000 * d + k)
    X = _minmax(rng, N, d)
    C = X[np.sort(rng.choice(N, k, replace=False))].copy()
    return X, C


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _step(ctx, X, C):
    """One single step, checked against the oracle's labels and NumPy's
    sequential sums (bit patterns: the sign of a zero too)."""
    k = C.shape[0]
    ctx.load_points(X)
    assert ctx.info()["mode"] == 2
    sums, counts = ctx.lloyd_step_f64(C)
    labels = ctx.labels()
    np.testing.assert_array_equal(labels, ko.assign(X, C))
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=k))
    np.testing.assert_array_equal(_bits(sums), _bits(_numpy_sums(X, labels, k)))
    return sums, counts, labels


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", range(2, 17))
def test_single_step_every_d(ctx, d, k):
    X, C = _case(d, k)
    _step(ctx, X, C)


@pytest.fixture(scope="module")
def shard_ctxs(ctx):
    import _cdr

    cs = [_cdr.Context(ctx.device) for _ in range(2)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", (2, 7, 16))
def test_device_run_and_shards(ctx, shard_ctxs, d, k):
    X, C = _case(d, k)
    sums, counts, labels = _step(ctx, X, C)
    # the device run's step (the label-change flags are written)
    _, applied, reason, means, run_counts = ctx.lloyd_f64_run(C, 1, -1.0)
    assert (applied, reason) == (1, ctx.F64_RUN_ALL)
    np.testing.assert_array_equal(ctx.labels(), labels)
    np.testing.assert_array_equal(run_counts, counts)
    assert (counts > 0).all()
    np.testing.assert_array_equal(_bits(means), _bits(sums / counts[:, None].astype(np.float64)))
    # two contexts, rows split inside a block
    for c, part in zip(shard_ctxs, (X[:SPLIT], X[SPLIT:])):
        c.load_points(part)
        assert c.info()["mode"] == 2
    for s, cn, _ in _f64_shards_step(shard_ctxs, C):
        np.testing.assert_array_equal(_bits(s), _bits(sums))
        np.testing.assert_array_equal(cn, counts)
    np.testing.assert_array_equal(np.concatenate([c.labels() for c in shard_ctxs]), labels)

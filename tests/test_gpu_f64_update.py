"""F64-mode centroid sums in parallel (csrc/f64sum.hip) against NumPy's
sequential row-order sums (`X[labels == j].mean(axis=0)`,
src/kmeans_plusplus.py:41) and against the serial kernel, plus a whole
k-means at n = 2M on min-max-normalised (non-grid) features against
oracle.kmeans_oracle.kmeans, bit for bit."""
import time

import numpy as np
import pytest

from oracle import kmeans_oracle as ko

pytestmark = pytest.mark.gpu


def _minmax(rng, n, d):
    """Features as compute_features writes them: min-max normalised doubles
    (full 53-bit mantissas, not on any power-of-two grid)."""
    raw = rng.gamma(2.0, 3.0, (n, d)) * rng.random(d) + rng.normal(0, 1, (n, d))
    return (raw - raw.min(axis=0)) / (raw.max(axis=0) - raw.min(axis=0))


def _numpy_sums(X, labels, k):
    out = np.zeros((k, X.shape[1]))
    for j in range(k):
        m = labels == j
        if m.any():
            out[j] = np.add.reduce(X[m], axis=0)  # row-sequential for d >= 2
    return out


def _check_step(ctx, X, C, monkeypatch):
    ctx.load_points(X)
    assert ctx.info()["mode"] == 2
    sums, counts = ctx.lloyd_step_f64(C)
    walked = ctx.f64_walked()
    labels = ctx.labels()
    np.testing.assert_array_equal(labels, ko.assign(X, C))
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=C.shape[0]))
    np.testing.assert_array_equal(sums, _numpy_sums(X, labels, C.shape[0]))
    monkeypatch.setenv("CDR_F64_SERIAL", "1")
    s2, c2 = ctx.lloyd_step_f64(C)
    monkeypatch.delenv("CDR_F64_SERIAL")
    assert ctx.f64_walked() == -1
    np.testing.assert_array_equal(s2, sums)
    return walked


def test_nonneg_features_few_walks(ctx, monkeypatch):
    rng = np.random.default_rng(1)
    X = _minmax(rng, 300_000, 5)
    C = X[rng.choice(X.shape[0], 8, replace=False)].copy()
    walked = _check_step(ctx, X, C, monkeypatch)
    blocks = -(-X.shape[0] // 256) * 8 * 5
    assert 0 <= walked < 0.05 * blocks, walked


def test_mixed_signs_and_negative_columns(ctx, monkeypatch):
    rng = np.random.default_rng(2)
    X = _minmax(rng, 100_000, 4) - 0.5
    X[:, 3] = -np.abs(X[:, 3]) - 1e-3
    X[::97, 1] = -0.0
    C = X[rng.choice(X.shape[0], 6, replace=False)].copy()
    _check_step(ctx, X, C, monkeypatch)


def test_tiny_clusters_and_signed_zero(ctx, monkeypatch):
    rng = np.random.default_rng(3)
    X = _minmax(rng, 5000, 3)
    X[:10] = [-0.0, 0.0, -0.0]
    X[10] = [50.0, 50.0, 50.0]                        # a one-member cluster
    C = np.vstack([X[:1], X[10:11], X[rng.choice(5000, 4, replace=False)]])
    C[0] = [-0.0, -0.0, -0.0]
    _check_step(ctx, X, C, monkeypatch)


def test_kmeans_2m_minmax_features_bit_exact(ctx):
    """The verdict's size: 2M files x 5 min-max features, k = 8, k-means++
    seeding + Lloyd to convergence (max_iter 60), against the oracle."""
    import kmeans_plusplus as kp

    rng = np.random.default_rng(4)
    X = _minmax(rng, 2_000_000, 5)
    np.random.seed(7)
    t0 = time.perf_counter()
    C, labels = kp.kmeans(X, 8, random_state=42, max_iter=60, context=ctx)
    dt = time.perf_counter() - t0
    np.random.seed(7)
    C_ref, labels_ref = ko.kmeans(X, 8, random_state=42, max_iter=60)
    np.testing.assert_array_equal(C, C_ref)
    np.testing.assert_array_equal(labels, labels_ref)
    # the step time with the parallel sums (reported in the test log)
    ctx.load_points(X)
    ctx.lloyd_step_f64(C)
    ctx.synchronize()
    t1 = time.perf_counter()
    for _ in range(5):
        ctx.lloyd_step_f64(C)
    ctx.synchronize()
    step = (time.perf_counter() - t1) / 5
    print(f"\nF64 2M x 5 k=8: kmeans {dt:.2f} s, one step {step * 1e3:.2f} ms, "
          f"walked blocks {ctx.f64_walked()}")


@pytest.mark.parametrize("n,d,k", [(120_000, 16, 64), (80_000, 20, 10), (60_000, 6, 70),
                                   (50_000, 2, 3), (70_001, 9, 33)])
def test_step_shapes_fused_and_separate(ctx, monkeypatch, n, d, k):
    """The fused assignment + block pass (d <= 16, k <= 64: f64_step_fused),
    the separate passes (d > 16) and the serial sums (k > 64), at ragged n:
    labels = the oracle's, sums = NumPy's sequential sums, = the serial kernel."""
    rng = np.random.default_rng(10 + d + k)
    X = _minmax(rng, n, d)
    C = X[rng.choice(n, k, replace=False)].copy()
    _check_step(ctx, X, C, monkeypatch)
    # a second step from moved centroids (the predictions of the first are not reused)
    C2 = C * 0.75 + 0.125
    _check_step(ctx, X, C2, monkeypatch)


def _f64_shards_step(ctxs, C):
    """cdr_dist.f64_sharded_sums over W contexts on one GPU, the two
    all-gathers (and the chain's broadcasts) done by device copies: every
    context's (sums, counts, status)."""
    import torch

    W = len(ctxs)
    k, d = C.shape
    kd = k * d

    def sync():
        for c in ctxs:
            c.synchronize()
        torch.cuda.synchronize()

    def gather(bufs, m):
        sync()
        for r in range(W):
            for q in range(W):
                if q != r:
                    bufs[q][r * m:(r + 1) * m].copy_(bufs[r][r * m:(r + 1) * m])
        torch.cuda.synchronize()

    tot = [torch.zeros(W * 8 * (kd + k), dtype=torch.uint8, device="cuda") for _ in ctxs]
    sizes = [c.f64s_begin(C, W, r, tot[r].data_ptr()) for r, c in enumerate(ctxs)]
    m0, m1 = int(sizes[0][0]), int(sizes[0][1])
    gather(tot, m0)
    prog = [torch.zeros(W * m1, dtype=torch.uint8, device="cuda") for _ in ctxs]
    for r, c in enumerate(ctxs):
        c.f64s_build(tot[r].data_ptr(), prog[r].data_ptr())
    gather(prog, m1)
    outs = [c.f64s_finish(tot[r].data_ptr(), prog[r].data_ptr()) for r, c in enumerate(ctxs)]
    if outs[0][2]:  # the rank chain (every context saw the same status)
        chain = [torch.zeros(16 * kd, dtype=torch.uint8, device="cuda") for _ in ctxs]
        for r, c in enumerate(ctxs):
            sync()
            c.f64s_chain(chain[r].data_ptr())
            sync()
            for q in range(W):
                if q != r:
                    chain[q].copy_(chain[r])
            torch.cuda.synchronize()
        outs = [(chain[r].view(torch.float64)[:kd].cpu().numpy().reshape(k, d), o[1], o[2])
                for r, o in enumerate(outs)]
    return outs


@pytest.mark.parametrize("n,d,k,W,force", [(300_000, 5, 16, 2, False), (700_001, 5, 7, 3, False),
                                           (1_000_000, 8, 33, 4, False),
                                           (300_000, 5, 16, 3, True)],
                         ids=["W2", "W3", "W4-k33", "W3-chain"])
def test_sharded_f64_sums_contexts(ctx, monkeypatch, n, d, k, W, force):
    """VERDICT r4 (missing 1): F64 mode (main.py's min-max features, off any
    grid) over rows sharded on W contexts: the shards' approximate totals
    all-gathered, each shard's program (rank 0 its exact walk; the others
    transfer runs + element lists) all-gathered and composed in rank order on
    every context.  Sums (the sequential row-order NumPy sums,
    kmeans_plusplus.py:41) and counts are bit-identical to the single
    context's and NumPy's for three Lloyd steps; "-chain" forces the exact
    rank chain instead (CDR_F64S_FORCE_CHAIN)."""
    import _cdr
    from cdr_dist import shard_rows

    if force:
        monkeypatch.setenv("CDR_F64S_FORCE_CHAIN", "1")
    rng = np.random.default_rng(n + d + k)
    X = _minmax(rng, n, d)
    C = X[np.sort(rng.choice(n, k, replace=False))].copy()
    ctx.load_points(X)
    ctxs = [_cdr.Context(ctx.device) for _ in range(W)]
    try:
        for r, c in enumerate(ctxs):
            b, m = shard_rows(n, W, r)
            c.load_points(X[b:b + m])
            assert c.info()["mode"] == 2
        for step in range(3):
            want_s, want_c = ctx.lloyd_step_f64(C)
            labels = ctx.labels()
            if step == 0:
                np.testing.assert_array_equal(want_s, _numpy_sums(X, labels, k))
            outs = _f64_shards_step(ctxs, C)
            for sums, counts, status in outs:
                assert status == (1 if force else 0), status
                np.testing.assert_array_equal(counts, want_c)
                np.testing.assert_array_equal(sums, want_s)
            np.testing.assert_array_equal(np.concatenate([c.labels() for c in ctxs]), labels)
            nz = want_c > 0
            C = C.copy()
            C[nz] = want_s[nz] / want_c[nz, None]
    finally:
        for c in ctxs:
            c.close()


def _host_steps(ctx, C, steps):
    """The host loop of src/kmeans_plusplus.py:33-46 over cdr_lloyd_step_f64
    (no empty clusters here): C <- sums / counts, `steps` times."""
    for _ in range(steps):
        sums, counts = ctx.lloyd_step_f64(C)
        assert (counts > 0).all()
        C = sums / counts[:, None].astype(np.float64)
    return C


def test_device_run_matches_host_steps(ctx):
    """cdr_lloyd_f64_run (the steps resident on the device: means and shift
    on the device) = the host loop of single steps, bit for bit, labels too;
    tol <= 0 applies every step."""
    rng = np.random.default_rng(21)
    X = _minmax(rng, 300_001, 5)
    ctx.load_points(X)
    C0 = X[rng.choice(X.shape[0], 16, replace=False)].copy()
    C_host = _host_steps(ctx, C0, 7)
    lab_host = ctx.labels()
    C_dev, applied, reason, means, counts = ctx.lloyd_f64_run(C0, 7, -1.0)
    assert (applied, reason) == (7, ctx.F64_RUN_ALL)
    np.testing.assert_array_equal(C_dev, C_host)
    np.testing.assert_array_equal(ctx.labels(), lab_host)
    # the last step's means and counts are kept: its means are the result
    np.testing.assert_array_equal(means, C_dev)
    np.testing.assert_array_equal(counts, np.bincount(lab_host, minlength=16))
    # in two calls (the run resumes from the centroids it returned)
    C_a, n_a, _, _, _ = ctx.lloyd_f64_run(C0, 3, -1.0)
    C_b, n_b, _, _, _ = ctx.lloyd_f64_run(C_a, 4, -1.0)
    assert (n_a, n_b) == (3, 4)
    np.testing.assert_array_equal(C_b, C_host)


@pytest.mark.parametrize("n,d,k,steps,oracle_steps", [(1_000_003, 5, 16, 25, 0),
                                                      (200_003, 5, 24, 12, 12),
                                                      (150_001, 9, 64, 12, 6)])
def test_device_run_transfer_cache(ctx, monkeypatch, n, d, k, steps, oracle_steps):
    """The device run's transfer cache (f64_step_fused, tcache): a block
    keeps its transfers while its labels and binade predictions stay, so
    converging blob data recomputes few blocks per step.  `steps` steps in one
    call, in two calls (3 + the rest: the second starts the cache again) and
    with the cache off (CDR_F64_TCACHE=0) give the same centroids and labels
    bit for bit, and so does the host loop of single steps (no cache).  The
    three shapes run the three f64_transfer instantiations through the
    dirty-block list (8, 7 and 6 transfers per thread: k <= 16, <= 32, <= 64);
    the k > 16 ones also equal the oracle's Lloyd steps on the same X."""
    gen = type(ctx)(0)
    try:
        gen.generate_points(n, 0, n, d, k, 0x5EED)
        X = gen.get_rows(np.arange(n, dtype=np.int64))
    finally:
        gen.close()
    X = (X - X.min(axis=0)) / (X.max(axis=0) - X.min(axis=0))
    ctx.load_points(X)
    assert ctx.info()["mode"] == 2
    C0 = X[np.sort(np.random.default_rng(42).choice(X.shape[0], k, replace=False))].copy()
    C_one, n_one, _, _, _ = ctx.lloyd_f64_run(C0, steps, -1.0)
    lab_one = ctx.labels()
    C_a, n_a, _, _, _ = ctx.lloyd_f64_run(C0, 3, -1.0)
    C_two, n_b, _, _, _ = ctx.lloyd_f64_run(C_a, steps - 3, -1.0)
    assert (n_one, n_a, n_b) == (steps, 3, steps - 3)
    np.testing.assert_array_equal(C_two, C_one)
    np.testing.assert_array_equal(ctx.labels(), lab_one)
    monkeypatch.setenv("CDR_F64_TCACHE", "0")
    C_off, _, _, _, _ = ctx.lloyd_f64_run(C0, steps, -1.0)
    monkeypatch.delenv("CDR_F64_TCACHE")
    np.testing.assert_array_equal(C_off, C_one)
    np.testing.assert_array_equal(ctx.labels(), lab_one)
    np.testing.assert_array_equal(_host_steps(ctx, C0, steps), C_one)
    np.testing.assert_array_equal(ctx.labels(), lab_one)
    if oracle_steps:
        C_ref, lab_ref, _, _ = ko.lloyd(X, C0, oracle_steps, -1.0)
        if oracle_steps < steps:  # (the reference's cost: n d k per step)
            C_one, n_one, _, _, _ = ctx.lloyd_f64_run(C0, oracle_steps, -1.0)
            assert n_one == oracle_steps
            lab_one = ctx.labels()
        np.testing.assert_array_equal(C_one, C_ref)
        np.testing.assert_array_equal(lab_one, lab_ref)


def test_device_run_hands_back_empty_cluster(ctx):
    """A cluster without members stops the run before that step is applied:
    C_out = the centroids the step started from, means / counts = the step's
    (counts 0 for the empty one), labels = its assignment (the oracle's)."""
    rng = np.random.default_rng(22)
    X = _minmax(rng, 120_000, 4)
    ctx.load_points(X)
    C0 = X[rng.choice(X.shape[0], 6, replace=False)].copy()
    C0[2] = 40.0  # far from every point: no members
    C_dev, applied, reason, means, counts = ctx.lloyd_f64_run(C0, 5, -1.0)
    assert (applied, reason) == (0, ctx.F64_RUN_HOST)
    np.testing.assert_array_equal(C_dev, C0)
    lab = ko.assign(X, C0)
    np.testing.assert_array_equal(ctx.labels(), lab)
    np.testing.assert_array_equal(counts, np.bincount(lab, minlength=6))
    assert counts[2] == 0
    sums, _ = ctx.lloyd_step_f64(C0)
    nz = counts > 0
    np.testing.assert_array_equal(means[nz], sums[nz] / counts[nz, None])


def test_device_run_stops_queueing_after_it_stops(ctx):
    """A run that converges early does not queue the rest of max_steps: the
    steps go to the device in chunks (4, 8, 16) with the state read between
    them, so at most one chunk (16 steps) runs after the stop (the
    dead steps' kernels cost ~0.5 ms each).  Queued steps are counted by the
    per-step profile."""
    rng = np.random.default_rng(24)
    X = _minmax(rng, 200_000, 5)
    ctx.load_points(X)
    C0 = X[rng.choice(X.shape[0], 8, replace=False)].copy()
    ctx.profile_reset(True, every=1)
    C_dev, applied, reason, _, _ = ctx.lloyd_f64_run(C0, 400, 1e-3)
    queued = ctx.profile_read()["steps"]
    ctx.profile_reset(False)
    assert reason in (ctx.F64_RUN_CONVERGED, ctx.F64_RUN_HOST)
    assert applied < 200
    assert applied <= queued <= applied + 1 + 16, (applied, queued)
    # the stopped run's result is the host loop's
    np.testing.assert_array_equal(C_dev, _host_steps(ctx, C0, applied))


@pytest.mark.parametrize("n,d,k,seed", [(200_000, 5, 6, 31), (150_000, 3, 12, 32)])
def test_kmeans_device_run_vs_oracle(ctx, n, d, k, seed):
    """kmeans() on F64 points runs the device loop to convergence (tol 1e-4,
    decided on the device, near-tol shifts by the host) and matches the
    oracle's reference loop bit for bit: centroids, labels.  Three far points
    give D^2 seeding a small cluster to pick."""
    import kmeans_plusplus as kp

    rng = np.random.default_rng(seed)
    X = _minmax(rng, n, d)
    X[:3] = 5.0  # three far points: their cluster empties after the first moves
    np.random.seed(seed)
    C, labels = kp.kmeans(X, k, random_state=seed, max_iter=40, context=ctx)
    np.random.seed(seed)
    C_ref, labels_ref = ko.kmeans(X, k, random_state=seed, max_iter=40)
    np.testing.assert_array_equal(C, C_ref)
    np.testing.assert_array_equal(labels, labels_ref)


def test_assign_screen_ties_duplicates_and_ranges(ctx, monkeypatch):
    """The fp32 screen in front of the exact argmin (k <= 16,
    f64_screen_argmin): grid points exactly between two centroids (the first
    index wins), a duplicated centroid (never chosen), points with a value
    below 2^-60 or above 2^60 (the exact pass alone) - labels equal the
    oracle's, sums NumPy's, and the same at k = 17 (no screen)."""
    rng = np.random.default_rng(23)
    X = _minmax(rng, 60_000, 4)
    X[:2000] = np.round(X[:2000] * 4) / 4
    X[2000:2100, 0] = 1e-30
    X[2100:2200, 1] = 3e20
    base = np.array([[0.25, 0.25, 0.25, 0.25], [0.75, 0.25, 0.25, 0.25], [0.25, 0.75, 0.25, 0.25],
                     [0.25, 0.25, 0.25, 0.25], [0.5, 0.5, 0.5, 0.5], [0.25, 0.25, 0.75, 0.75]])
    C = np.vstack([base, X[rng.choice(np.arange(2200, 60_000), 10, replace=False)]])
    assert C.shape[0] == 16
    _check_step(ctx, X, C, monkeypatch)
    C17 = np.vstack([C, X[2200:2201]])
    _check_step(ctx, X, C17, monkeypatch)


def _gloo_f64_worker(rank, world, port, out_dir):
    import os

    import torch.distributed as dist

    from _cdr import Context
    from cdr_dist import Comm, ShardedLloyd

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    X = np.load(os.path.join(out_dir, "X.npy"))
    ctx = Context(0)
    ctx.load_points(X)
    msg = "no error"
    try:
        ShardedLloyd(ctx, Comm(dist, None), X.shape[0], 0)
    except NotImplementedError as e:
        msg = "NotImplementedError: " + str(e)
    with open(os.path.join(out_dir, f"r{rank}.txt"), "w") as fh:
        fh.write(msg)
    ctx.close()
    dist.destroy_process_group()


def test_sharded_f64_on_gloo_raises_clearly(tmp_path):
    """F64 points on a real GPU context under gloo (host buffers): the
    sharded F64 sums cannot run there, and ShardedLloyd says so up front
    instead of failing inside ctypes."""
    from test_features_dist import _free_port

    mp = pytest.importorskip("torch.multiprocessing")
    rng = np.random.default_rng(25)
    np.save(tmp_path / "X.npy", _minmax(rng, 20_000, 4))
    mp.spawn(_gloo_f64_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    msg = (tmp_path / "r0.txt").read_text()
    assert msg.startswith("NotImplementedError") and "nccl" in msg, msg

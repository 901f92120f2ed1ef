"""The bounded screen's work distribution at small sizes (screen32bs16,
DESIGN.md 4.3g): generation regions and the dynamic tail switch on by
themselves only from about 1M and 50M points, so the test switches
CDR_S32BS_CUS (the grid of a device with that many CUs) and
CDR_S32BS_DYN_MIN (the tail's chunks-per-wave threshold) bring them down to
ragged chunk counts, pools of a chunk or two and waves with nothing to
stream.

A chunk nobody streams leaves stale labels the next step may repair, and a
chunk streamed twice applies its moves twice to the running sums, so every
step is checked, not the last one: all labels against the oracle's
assignment from the previous centroids and the new centroids against
X[labels == j].mean(axis=0), bit for bit (src/kmeans_plusplus.py:33-41).
Each case first asserts through Context.screen_layout() that the intended
path ran.

Sensitivity, checked once on an MI355X with two scratch builds that only skip
work: every XCD pool one chunk short (P1 - 1) fails (a) and (b) on the
labels of step 2 (3841 of 131001 and 2720 of 225001 wrong); block 0 not
zeroing the other parity's counters fails (f) on the second loop's labels
(11634 of 131001 wrong)."""
import functools
import time

import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from oracle import synth
from test_gpu_loop import _grid_uniform, _loop, _mirrored

pytestmark = pytest.mark.gpu

N_A = 131_072 - 71  # 256 chunks of 512 points, the last one ragged


def _data(kind, n, d, k):
    """Points and start centroids as test_bounded_screen_many_steps_vs_oracle
    draws them (mirror: an even number of rows, n - n % 2)."""
    if kind == "blobs":
        X = synth.generate(n, 0, n, d, k, 17 * n + d)
    elif kind == "uniform":
        X = _grid_uniform(n, d, n + d)
    else:
        X = _mirrored(n, d, k, n + d)
    rng = np.random.default_rng(k + d)
    if kind == "mirror":
        half = X[n // 50 + rng.choice(n // 2 - n // 50, k // 2, replace=False)]
        C0 = np.concatenate([half, 1.0 - half])
    else:
        C0 = X[np.sort(rng.choice(X.shape[0], k, replace=False))]
    return X, C0


def _reference(kind, n, d, k, steps):
    """X, C0 and the oracle's (labels, new centroids) of every step."""
    X, C0 = _data(kind, n, d, k)
    t0 = time.perf_counter()
    np.random.seed(3)
    C, traj = C0, []
    for _ in range(steps):
        lab = ko.assign(X, C)
        C = ko.update(X, lab, C, X.shape[0])
        traj.append((lab, C))
    print(f"\nreference {kind} {X.shape[0]} x {d}, k = {k}, {steps} steps: "
          f"{time.perf_counter() - t0:.1f} s")
    for a in (X, C0):
        a.setflags(write=False)
    return X, C0, traj


# (a) and (d) share their references: computed once, read only
_reference_a = functools.lru_cache(maxsize=3)(_reference)


def _device_steps(ctx, X, C0, steps):
    """`steps` device-loop steps enqueued one at a time: the labels and
    centroids after each, and the bounded screen's layout at the end."""
    from cdr_dist import DeviceLloyd

    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, np.array(C0, dtype=np.float64), -1.0, lambda g: X[g], X.shape[0])
    out, layouts = [], []
    try:
        for s in range(steps):
            assert run.advance(1) == 1
            out.append((ctx.labels(), ctx.lloyd_read()[0]))
            if s >= 2:  # step 3 is the first bounded step after the rebuild
                assert ctx.profile_kernel().startswith("screen32bs16<"), ctx.profile_kernel()
                layouts.append(ctx.screen_layout())
    finally:
        ctx.lloyd_end()
    # every bounded launch of the run had the same layout
    assert all(l == layouts[0] for l in layouts), layouts
    return out, layouts[0]


def _check_every_step(got, traj):
    for s, ((lab, C), (lab_ref, C_ref)) in enumerate(zip(got, traj)):
        np.testing.assert_array_equal(lab, lab_ref, err_msg=f"labels of step {s + 1}")
        np.testing.assert_array_equal(C, C_ref, err_msg=f"centroids of step {s + 1}")


def _switches(monkeypatch, cus=None, dyn_min=None):
    monkeypatch.setenv("CDR_BOUNDS", "1")
    monkeypatch.setenv("CDR_S32B_SPLIT", "1")
    monkeypatch.setenv("CDR_S32BS_SPLIT", "0")
    for name, v in (("CDR_S32BS_CUS", cus), ("CDR_S32BS_DYN_MIN", dyn_min)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


F_BLOBS, F_SEED = 35, 1  # (blobs, seed) whose run from _farthest_first takes more than 2 steps


def _farthest_first(X, k):
    """Row 0, then k - 1 times the row farthest from the rows picked: one
    start centroid per separated blob, so the loop converges in a few steps."""
    idx = [0]
    dmin = ((X - X[0]) ** 2).sum(axis=1)
    for _ in range(1, k):
        idx.append(int(np.argmax(dmin)))
        dmin = np.minimum(dmin, ((X - X[idx[-1]]) ** 2).sum(axis=1))
    return X[np.array(idx)].copy()


# the headline template screen32bs16<4,2> (d = 13..16, k = 33..64); no cluster
# empties in these runs, so the loop never stops for the host
CASES_A = [("uniform", 16, 40), ("mirror", 13, 34), ("blobs", 15, 38)]
LAYOUT_A = {"workgroups": 32, "slot_wg": 8, "dyn_pct": 90, "max_chunks": 3, "nchunks": 256,
            "word_bytes": 2}


@pytest.mark.parametrize("kind,d,k", CASES_A)
def test_regions_and_dynamic_tail_small_pools(ctx, monkeypatch, kind, d, k):
    """(a) 8 CUs' grid (32 workgroups) over 256 chunks: regions of 73 / 67 /
    61 / 55 chunks, 2 static chunks per wave, pools of 9 / 3 / 0 / 0 chunks
    split over 8 XCDs (one or two chunks, less than a group, or none: the
    first claim may find the pool spent).  7 steps from the start: the full
    screen, the bound rebuild, the first bounded step (every word fails: the
    dense loop takes over while claiming), then steady steps with a rebase."""
    X, C0, traj = _reference_a(kind, N_A, d, k, 7)
    _switches(monkeypatch, cus=8, dyn_min=2)
    got, layout = _device_steps(ctx, X, C0, 7)
    assert layout == LAYOUT_A, layout
    _check_every_step(got, traj)


@pytest.mark.parametrize("kind,d,k", CASES_A)
def test_regions_without_dynamic_tail(ctx, monkeypatch, kind, d, k):
    """(d) The same regions streamed statically (the tail's threshold at its
    default): every step equals the oracle's and run (a)'s, bit for bit."""
    X, C0, traj = _reference_a(kind, N_A, d, k, 7)
    _switches(monkeypatch, cus=8)
    got, layout = _device_steps(ctx, X, C0, 7)
    assert layout == dict(LAYOUT_A, dyn_pct=100), layout
    _check_every_step(got, traj)
    _switches(monkeypatch, cus=8, dyn_min=2)
    got_a, layout_a = _device_steps(ctx, X, C0, 7)
    assert layout_a == LAYOUT_A, layout_a
    _check_every_step(got, got_a)


def test_pools_of_whole_and_partial_groups(ctx, monkeypatch):
    """(b) 448 chunks: regions of 128 / 118 / 106 / 96, static 96 / 96 / 64 /
    64, pools of 32 / 22 / 42 / 32: per XCD 4 chunks (one whole group), 2-3
    and 5-6 (a group and a remainder of one or two)."""
    n, d, k = 229_376 - 4_375, 8, 16
    X, C0, traj = _reference("uniform", n, d, k, 7)
    _switches(monkeypatch, cus=8, dyn_min=3)
    got, layout = _device_steps(ctx, X, C0, 7)
    assert layout == {"workgroups": 32, "slot_wg": 8, "dyn_pct": 90, "max_chunks": 4,
                      "nchunks": 448, "word_bytes": 2}, layout
    _check_every_step(got, traj)


def test_several_static_groups_per_wave(ctx, monkeypatch):
    """(c) 1184 chunks: regions of 340 / 311 / 281 / 252, 9 / 8 / 7 / 7
    static chunks per wave (two full groups of 4 and one chunk, two full
    groups, one full group and three chunks), then claimed groups."""
    n, d, k = 606_208 - 6_209, 6, 12
    X, C0, traj = _reference("uniform", n, d, k, 7)
    _switches(monkeypatch, cus=8, dyn_min=4)
    got, layout = _device_steps(ctx, X, C0, 7)
    assert layout == {"workgroups": 32, "slot_wg": 8, "dyn_pct": 90, "max_chunks": 11,
                      "nchunks": 1184, "word_bytes": 2}, layout
    _check_every_step(got, traj)


def test_real_grid_mostly_idle_waves(ctx, monkeypatch):
    """(e) No switches: the smallest point count whose grid is full (1024
    workgroups, 4096 waves) has 2064 chunks, so in every region most waves
    stream one chunk or none and the prefetch clamps at the last chunk."""
    n, d, k = 1_048_576 + 5_000, 3, 7
    X, C0, traj = _reference("uniform", n, d, k, 7)
    _switches(monkeypatch)
    got, layout = _device_steps(ctx, X, C0, 7)
    assert layout == {"workgroups": 1024, "slot_wg": 256, "dyn_pct": 100, "max_chunks": 1,
                      "nchunks": 2064, "word_bytes": 2}, layout
    _check_every_step(got, traj)


def test_counter_parities_across_gated_launches_and_a_second_loop(ctx, monkeypatch):
    """(f) The tail's counters have two parities; every launch zeroes the
    other one's for the next launch, before its gate.  A loop run to tol
    queues steps beyond convergence (launches that return at the gate), then
    a second loop on the same context starts from other centroids: both
    equal the oracle (labels, centroids, the first run's step count)."""
    d, k = 13, 33
    X = synth.generate(N_A, 0, N_A, d, F_BLOBS, F_SEED)
    C0 = _farthest_first(X, k)
    _switches(monkeypatch, cus=8, dyn_min=2)
    ctx.load_points(X)
    np.random.seed(5)
    C, st = _loop(ctx, C0, 40, 1e-4, X)
    lab = ctx.labels()
    assert ctx.screen_layout() == LAYOUT_A, ctx.screen_layout()
    np.random.seed(5)
    C_ref, lab_ref, _, steps = ko.lloyd(X, C0, 40, 1e-4)
    assert 2 < st["steps"] == steps < st["enqueued"], (st, steps)  # gated launches followed
    np.testing.assert_array_equal(lab, lab_ref)
    np.testing.assert_array_equal(C, C_ref)
    C0b = X[np.sort(np.random.default_rng(9).choice(N_A, k, replace=False))]
    np.random.seed(6)
    C, st = _loop(ctx, C0b, 5, -1.0, X)
    assert st["steps"] == 5 and ctx.screen_layout() == LAYOUT_A
    np.random.seed(6)
    C_ref, lab_ref, _, _ = ko.lloyd(X, C0b, 5, -1.0)
    np.testing.assert_array_equal(ctx.labels(), lab_ref)
    np.testing.assert_array_equal(C, C_ref)

"""Every (Q, MT) arm of the screen32 families' dispatch (csrc/screen32_common.h):
Q = 1..4 feature quads (d = 3, 7, 11, 16) times MT = 1, 2 centroid tiles
(k = 20, 40), on the full screen, the pruned screen, the bounded screen in
its queue form (screen32b), its two-launch form (screen32bz + screen32bs) and
the fused default (screen32bs16).  The other small-size tests do not reach
Q = 3, Q = 4 with MT = 1 or Q = 1 with MT = 2 on a DELTA kernel, so a
transposed or missing arm there would go unseen.

n = 24,539 rows: 48 chunks of 512, the last one ragged.  On the CPU oracle
(np.random.seed(3), six steps) no cluster empties in any of the eight shapes
(smallest count 97) and 1,000 to 6,300 points change label at every step, so
the device loop never stops for the host and the move path runs each step.

Every step's labels and centroids (host-plan path: int64 sums) must equal the
oracle's bit for bit, and the kernel name Context.profile_kernel() reports
must equal the expected instantiation exactly: a prefix test would pass a
transposed arm."""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from test_gpu_screen_layout import _check_every_step, _data, _switches

pytestmark = pytest.mark.gpu

N = 24_576 - 37  # 48 chunks of 512 points, the last one ragged
STEPS = 5
SCALE_BITS = 24  # the 2^-24 grid of _grid_uniform
SHAPES = [(d, k) for d in (3, 7, 11, 16) for k in (20, 40)]


@functools.lru_cache(maxsize=len(SHAPES))
def _reference(d, k):
    """X, C0 and the oracle's (labels, new centroids, int64 partials) of
    every step: computed once per shape, shared by the four paths, read only."""
    X, C0 = _data("uniform", N, d, k)
    np.random.seed(3)
    C, traj = C0, []
    for _ in range(STEPS):
        lab, out = ko.lloyd_partials(X, C, SCALE_BITS)
        C = ko.update(X, lab, C, X.shape[0])
        for a in (lab, out, C):
            a.setflags(write=False)
        traj.append((lab, C, out))
    for a in (X, C0):
        a.setflags(write=False)
    return X, C0, traj


def _qmt(d, k):
    return (d + 3) // 4, 1 if k <= 32 else 2


@pytest.mark.parametrize("d,k", SHAPES)
def test_host_plan_full_then_pruned(ctx, d, k):
    """Host-plan steps (Context.lloyd_step): the full screen, then the pruned
    screen with its fused fixup."""
    X, C0, traj = _reference(d, k)
    Q, MT = _qmt(d, k)
    QH = 1 if Q <= 2 else 2
    fullq = "true" if Q == 2 * QH else "false"
    ctx.load_points(X)
    info = ctx.info()
    assert info["scale_bits"] == SCALE_BITS, info
    C = C0
    for s, (lab_ref, C_ref, out_ref) in enumerate(traj):
        out = ctx.lloyd_step(np.array(C, dtype=np.float64))
        name = ctx.profile_kernel()
        print(f"step {s + 1}: {name}")
        if s == 0:  # (PRE: grid data in the unit cube has an exact pre-centred copy)
            assert name == f"screen32<{QH},{MT},{fullq},false,false,true>", name
        else:
            assert name == f"screen32p<{Q},{MT},3>+fixup", name
        np.testing.assert_array_equal(ctx.labels(), lab_ref, err_msg=f"labels of step {s + 1}")
        np.testing.assert_array_equal(out, out_ref, err_msg=f"sums of step {s + 1}")
        C = C_ref


def _device_steps_named(ctx, X, C0, want):
    """STEPS device-loop steps enqueued one at a time: labels and centroids
    after each; from step 3 on (the first bounded step after the rebuild)
    the kernel name must equal `want`."""
    from cdr_dist import DeviceLloyd

    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, np.array(C0, dtype=np.float64), -1.0, lambda g: X[g], X.shape[0])
    out = []
    try:
        for s in range(STEPS):
            assert run.advance(1) == 1
            out.append((ctx.labels(), ctx.lloyd_read()[0]))
            name = ctx.profile_kernel()
            print(f"step {s + 1}: {name}")
            if s >= 2:
                assert name == want, (name, want)
    finally:
        ctx.lloyd_end()
    return out


def _device_case(ctx, monkeypatch, d, k, want, **env):
    X, C0, traj = _reference(d, k)
    _switches(monkeypatch)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    got = _device_steps_named(ctx, X, C0, want.format(*_qmt(d, k)))
    _check_every_step(got, [(lab, C) for lab, C, _ in traj])


@pytest.mark.parametrize("d,k", SHAPES)
def test_device_loop_fused_bounded(ctx, monkeypatch, d, k):
    """The default: 2-byte bound words, deciding in registers."""
    _device_case(ctx, monkeypatch, d, k, "screen32bs16<{},{}>")


@pytest.mark.parametrize("d,k", SHAPES)
def test_device_loop_queue_bounded(ctx, monkeypatch, d, k):
    """CDR_S32B_SPLIT=0: screen32b (LDS queue, fused fixup)."""
    _device_case(ctx, monkeypatch, d, k, "screen32b<{},{}>+fixup", CDR_S32B_SPLIT="0")


@pytest.mark.parametrize("d,k", SHAPES)
def test_device_loop_two_launch_bounded(ctx, monkeypatch, d, k):
    """CDR_S32BS_SPLIT=1: screen32bz lists the failed points, screen32bs
    decides the lists."""
    _device_case(ctx, monkeypatch, d, k, "screen32bs<{},{}>split", CDR_S32BS_SPLIT="1")

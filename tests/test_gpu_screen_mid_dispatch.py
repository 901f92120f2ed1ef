"""Every reachable arm of the medium screens' launch tables (csrc/screen_mid.hip):
screen_fast<DCH, KT> x NONNEG x FULL (registers hold the fragments: KT * DCH
<= 4) and screen_kernel<DCH> in its PACK6 (KT <= 4) and tile-index forms, the
last shape the screen takes (d = 64, k = 63: 65,528 of 65,536 bytes of LDS),
the first one it leaves to the next path of the step (k = 64: 66,048 bytes),
and the exact fallback of both families on points that tie.  The other
small-size tests reach screen_fast<2,1>, <2,2>, <4,1> and screen_kernel<1>,
<2>, <4> only, so a transposed or missing arm elsewhere would go unseen.

n = 24,539 rows of the 2^-24 grid (test_gpu_screen_layout._data "uniform").
d > 16 keeps every shape off screen32.  Two host-plan steps per case, the
second from the oracle's updated centroids: labels and int64 sums must equal
the oracle's bit for bit, and the kernel name Context.profile_kernel() reports
must equal the expected instantiation exactly.

The same points minus 0.5 are still on the grid and have negative minima:
screen_fast then adds sign-extended values (NONNEG false).  The second shape
of every screen_fast pair has d4 == 16 * DCH (FULL: no masked quad loads)."""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from test_gpu_screen_layout import _data

pytestmark = pytest.mark.gpu

N = 24_576 - 37
STEPS = 2
SCALE_BITS = 24  # the 2^-24 grid of _grid_uniform
MODE_F32X = 1    # include/cdr.h CDR_MODE_F32X

# (d, k, DCH, KT); the second of each pair is the FULL form
FAST = [(20, 9, 2, 1), (32, 16, 2, 1), (24, 20, 2, 2), (32, 32, 2, 2),
        (40, 12, 3, 1), (48, 16, 3, 1), (50, 10, 4, 1), (64, 16, 4, 1)]
# (d, k, DCH): (16, 240) fills 63,360 bytes; (24, 33) and (40, 24) have
# KT <= 4 (PACK6); (64, 63) is the last shape the screen takes
KERNEL = [(3, 100, 1), (16, 240, 1), (24, 33, 2), (24, 70, 2),
          (40, 24, 3), (40, 70, 3), (64, 24, 4), (64, 63, 4)]


@functools.lru_cache(maxsize=None)
def _reference(d, k, shifted=False, tie=False):
    """X, C0 and the oracle's (labels, new centroids, int64 partials) of both
    steps: computed once per case, read only."""
    X, C0 = _data("uniform", N, d, k)
    if shifted:
        X, C0 = X - 0.5, C0 - 0.5
    if tie:
        C0 = C0.copy()
        C0[1] = C0[0]  # every point nearest centroid 0 ties with centroid 1
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


def _two_steps(ctx, X, C0, traj, check_name):
    """Both steps against the oracle; the fallback count of each step."""
    ctx.load_points(X)
    info = ctx.info()
    assert info["mode"] == MODE_F32X, info
    assert info["scale_bits"] == SCALE_BITS, info
    C, fallbacks = C0, []
    for s, (lab_ref, C_ref, out_ref) in enumerate(traj):
        out = ctx.lloyd_step(np.array(C, dtype=np.float64))
        name = ctx.profile_kernel()
        fallbacks.append(ctx.fallback_count())
        print(f"step {s + 1}: {name}, {fallbacks[-1]} fallback points")
        check_name(name)
        np.testing.assert_array_equal(ctx.labels(), lab_ref, err_msg=f"labels of step {s + 1}")
        np.testing.assert_array_equal(out, out_ref, err_msg=f"sums of step {s + 1}")
        C = C_ref
    return fallbacks


def _named(want):
    def check(name):
        assert name == want, (name, want)
    return check


@pytest.mark.parametrize("shifted", [False, True], ids=["nonneg", "negative"])
@pytest.mark.parametrize("d,k,DCH,KT", FAST)
def test_screen_fast_arm(ctx, d, k, DCH, KT, shifted):
    X, C0, traj = _reference(d, k, shifted)
    assert (X.min() < 0.0) == shifted
    _two_steps(ctx, X, C0, traj, _named(f"screen_fast<{DCH},{KT}>"))


@pytest.mark.parametrize("d,k,DCH", KERNEL)
def test_screen_kernel_arm(ctx, d, k, DCH):
    X, C0, traj = _reference(d, k)
    _two_steps(ctx, X, C0, traj, _named(f"screen_kernel<{DCH}>"))


def test_first_shape_past_the_medium_screen(ctx):
    """d = 64, k = 64 needs 66,048 bytes of LDS: the medium screen refuses it
    and the step's next path decides the labels."""
    X, C0, traj = _reference(64, 64)

    def check(name):
        assert not name.startswith(("screen_kernel", "screen_fast")), name

    _two_steps(ctx, X, C0, traj, check)


@pytest.mark.parametrize("d,k,want", [(24, 20, "screen_fast<2,2>"), (24, 70, "screen_kernel<2>")])
def test_tied_points_take_the_exact_fallback(ctx, d, k, want):
    """C0[1] == C0[0]: no point nearest that centroid can be certified, the
    exact fallback gives each of them the first index."""
    X, C0, traj = _reference(d, k, tie=True)
    tied = int(np.count_nonzero(traj[0][0] == 0))
    assert tied > 0 and not np.any(traj[0][0] == 1)
    fallbacks = _two_steps(ctx, X, C0, traj, _named(want))
    assert fallbacks[0] >= tied, (fallbacks, tied)

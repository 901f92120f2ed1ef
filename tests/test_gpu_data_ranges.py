"""GPU parity on data outside the unit cube (tests/data_families.py): the
storage mode and scale the gate chooses (decide_mode, csrc/cdr_runtime.hip),
k-means++ seeding, one Lloyd step, the device loop and the drop-in kmeans(),
bit for bit against oracle.kmeans_oracle.

The families leave the geometry every other parity test uses ([0, 1) on the
2^-24 grid, or min-max doubles): scales S = 0, 12, 14, 126, a screen transform
with sigma = -11 or -5, negative minima (screen_fast's signed variant),
constant columns, duplicated rows, and two families whose pre-centred fp32
copy is not exact, so that screen32<..., PRE = false> and split_copy_kernel
round fma(x, 2^sigma, -mu 2^sigma) and large k has no screen_big.
tests/test_data_families.py checks the families' own properties on the CPU.
"""
import numpy as np
import pytest

import data_families as df
from oracle import kmeans_oracle as ko
from test_gpu_f64_update import _numpy_sums
from test_gpu_loop import _loop

pytestmark = pytest.mark.gpu

RS = df.SEED_RANDOM_STATE


def _expected_kernel(name, d, k, want):
    """The first step's screen kernel where its name encodes the path."""
    pre = "true" if want[2] else "false"
    if d <= 16 and k <= 64:
        q4 = (d + 3) // 4
        qh, mt = (1 if q4 <= 2 else 2), (1 if k <= 32 else 2)
        full = "true" if q4 == 2 * qh else "false"
        return ("screen32<%d,%d,%s,false,false,%s>" % (qh, mt, full, pre),)
    kt, dch = (k + 15) // 16, (d + 15) // 16
    if k * (d + 1) * 8 + kt * dch * 2 * 64 * 16 <= 64 * 1024:  # the host-plan screens (screen_mid.hip)
        return ("screen_fast<%d,%d>" % (dch, kt) if kt * dch <= 4 else "screen_kernel<%d>" % dch,)
    if want[2]:
        return ("screen_big",)
    return ("assign_exact",)  # no screen takes it: exact fp64 distances for every point


@pytest.mark.parametrize("case", df.CASES, ids=df.case_id)
def test_family_parity(ctx, case):
    import kmeans_plusplus as kp

    name, n, d, k = case
    X, ref, want = df.data(case), df.reference(case), df.EXPECT[name]
    steps = df.loop_steps(k)

    # mode
    ctx.load_points(X)
    info = ctx.info()
    print(f"\n{df.case_id(case)}: mode {info['mode']} scale_bits {info['scale_bits']}")
    if want is not None:
        assert (info["mode"], info["scale_bits"]) == want[:2], info
    f32x = info["mode"] == df.MODE_F32X

    # seeding
    C0 = kp.kmeans_plusplus_init(X, k, random_state=RS, context=ctx)
    np.testing.assert_array_equal(C0, ko.kmeans_plusplus_init(X, k, random_state=RS))
    np.testing.assert_array_equal(C0, ref["C0"])

    # one step from the seeds
    if f32x:
        out = ctx.lloyd_step(C0)
        kernel = ctx.profile_kernel()
        print(f"{df.case_id(case)}: first step {kernel}")
        want_labels, want_out = ko.lloyd_partials(X, C0, info["scale_bits"])
        np.testing.assert_array_equal(ctx.labels(), want_labels)
        np.testing.assert_array_equal(out, want_out)
        if want is not None:
            names = _expected_kernel(name, d, k, want)
            assert kernel.startswith(names), (kernel, names)
        if want is not None and d <= 16 and k <= 64:
            assert kernel.startswith("screen32<") and kernel.endswith(
                ",false>" if name in ("wide_int", "outlier") else ",true>"), kernel
    else:
        sums, counts = ctx.lloyd_step_f64(C0)
        print(f"{df.case_id(case)}: first step {ctx.profile_kernel()}")
        labels = ctx.labels()
        np.testing.assert_array_equal(labels, ko.assign(X, C0))
        np.testing.assert_array_equal(counts, np.bincount(labels, minlength=k))
        np.testing.assert_array_equal(sums, _numpy_sums(X, labels, k))

    # the loop (no cluster runs empty: test_data_families.py, so no reseed draw)
    C_ref, lab_ref = ref["C"], ref["labels"][-1]
    if f32x:
        C, st = _loop(ctx, C0, steps, -1.0, X)
        assert st["steps"] == steps
        print(f"{df.case_id(case)}: loop's last step {ctx.profile_kernel()}")
    elif d <= 16 and k <= 64:
        C, applied, reason, _, _ = ctx.lloyd_f64_run(C0, steps, -1.0)
        assert (applied, reason) == (steps, ctx.F64_RUN_ALL)
    else:  # (the resident F64 run takes d <= 16, k <= 64: single steps, host division)
        C = C0
        for _ in range(steps):
            sums, counts = ctx.lloyd_step_f64(C)
            C = sums / counts[:, None].astype(np.float64)
    np.testing.assert_array_equal(ctx.labels(), lab_ref)
    np.testing.assert_array_equal(C, C_ref)


@pytest.mark.parametrize("name", df.FAMILIES)
def test_family_kmeans_end_to_end(ctx, name):
    """The drop-in kmeans() (seeding, loop, tol) against the oracle's."""
    import kmeans_plusplus as kp

    n, d, k = df.SHAPES_ALL
    X = np.array(df.data((name, n, d, k)))
    np.random.seed(3)
    C, lab = kp.kmeans(X, k, random_state=RS, max_iter=4, context=ctx)
    np.random.seed(3)
    C_ref, lab_ref = ko.kmeans(X, k, random_state=RS, max_iter=4)
    np.testing.assert_array_equal(lab, lab_ref)
    np.testing.assert_array_equal(C, C_ref)

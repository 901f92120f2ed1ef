"""The exact sequential sums of csrc/f64sum.hip on the designed sequences of
tests/f64sum_cases.py (rounding ties inside composed transfers, exact
power-of-two landings, subnormal binades, signed and cancelling running
values, large exponents, an overflowing sum, the fp32 instance), through
every product form: lloyd_step_f64 fused / separate / serial, the device run
with and without the transfer cache, the sharded programs and their rank
chain, lloyd_step_f32r in both storage modes.  Everything is compared bit
for bit with ko.assign, np.bincount and NumPy's sequential sums.

The element-by-element walk is always right, so a wrong transfer could hide
behind it: every test also bounds ctx.f64_walked() — by the model's count
(tests/f64sum_cases.model_walk) plus one block per sequence where the running
value keeps its binade, by 5 % of the (block, sequence) pairs where it crosses
binades; the families that exist to be walked only need walked > 0."""
import functools

import numpy as np
import pytest

import f64sum_cases as fc
from oracle import kmeans_oracle as ko
from test_gpu_f64_update import _f64_shards_step, _numpy_sums

pytestmark = pytest.mark.gpu

FORM_IDS = ["fused-k2", "fused-k20", "fused-k40", "separate-d17", "serial-k70"]
MODEL_CAP = ("pinned_ties", "large", "large_sel", "large_inf", "f32_pinned_x", "f32_pinned_d")
PAIRS_CAP = ("growing_ties", "landings", "f32_growing_x", "f32_growing_d")


@functools.lru_cache(maxsize=None)
def _oracle_labels(fam, d, k):
    c = fc.case(fam, d, k)
    with np.errstate(over="ignore"):
        lab = ko.assign(c["X"], c["C"])
    lab.setflags(write=False)
    return lab


def _equal_bits(got, want):
    np.testing.assert_array_equal(got, want)  # (inf == inf)
    np.testing.assert_array_equal(np.signbit(got), np.signbit(want))


def _check_walked(fam, d, k, walked):
    seqs = fc.walks(fam, d, k)  # (the sequences that have members)
    model = sum(x.walked for x in seqs.values())
    pairs = fc.pairs(fam, d, k)
    print("\n%s d=%d k=%d: walked blocks device %d, model %d, of %d pairs" % (
        fam, d, k, walked, model, pairs))
    assert walked > 0
    if fam in MODEL_CAP:
        assert walked <= model + len(seqs), (walked, model, len(seqs))
    elif fam in PAIRS_CAP:
        assert walked < 0.05 * pairs, (walked, pairs)


@pytest.mark.parametrize("d,k", fc.SHAPES, ids=FORM_IDS)
@pytest.mark.parametrize("fam", fc.F64_FAMILIES)
def test_step_every_form(ctx, monkeypatch, fam, d, k):
    c = fc.case(fam, d, k)
    X, C = c["X"], c["C"]
    ctx.load_points(X)
    assert ctx.info()["mode"] == 2
    serial = k > 64
    if serial:
        monkeypatch.setenv("CDR_F64_SERIAL", "1")
    sums, counts = ctx.lloyd_step_f64(C)
    walked = ctx.f64_walked()
    labels = ctx.labels()
    np.testing.assert_array_equal(labels, _oracle_labels(fam, d, k))
    np.testing.assert_array_equal(labels, c["labels"])
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=k))
    with np.errstate(over="ignore"):
        want = _numpy_sums(X, labels, k)
    _equal_bits(want, c["sums"])
    _equal_bits(sums, want)
    if serial:
        assert walked == -1
        return
    _check_walked(fam, d, k, walked)
    monkeypatch.setenv("CDR_F64_SERIAL", "1")
    s2, c2 = ctx.lloyd_step_f64(C)
    monkeypatch.delenv("CDR_F64_SERIAL")
    assert ctx.f64_walked() == -1
    _equal_bits(s2, sums)
    np.testing.assert_array_equal(c2, counts)


RUN_SHAPES = [(3, 2), (5, 20), (4, 40)]


@pytest.mark.parametrize("d,k", RUN_SHAPES, ids=FORM_IDS[:3])
@pytest.mark.parametrize("fam", ["pinned_run", "signs_run"])
def test_device_run_with_and_without_transfer_cache(ctx, monkeypatch, fam, d, k):
    """cdr_lloyd_f64_run for 1, 2 and 3 steps = the host loop of single
    steps (centroids, labels, counts), with the transfer cache and with
    CDR_F64_TCACHE=0, on pinned_ties' and signs' sequences behind a selector
    of 10^6 (j + 1), which keeps every label in every step (asserted).  The
    rows of every sequence are then the same in steps 2 and 3, so a block is
    formed again only where an approximate block sum moved a prediction, and
    the last step's sums are step 1's: NumPy's.  The walked blocks of the last
    step are bounded as for a single step: for pinned_run by the model's count
    plus one block per sequence; for signs_run by twice the model's count
    (every block the model walks is a crossing or a flagged block, next to
    which a prediction can miss one more block)."""
    c = fc.case(fam, d, k)
    ctx.load_points(c["X"])
    assert ctx.info()["mode"] == 2
    C, host = c["C"], []
    for step in range(3):
        sums, counts = ctx.lloyd_step_f64(C)
        _equal_bits(sums, c["sums"])
        np.testing.assert_array_equal(ctx.labels(), c["labels"])  # frozen
        np.testing.assert_array_equal(counts, np.bincount(c["labels"], minlength=k))
        C = sums / counts[:, None].astype(np.float64)
        host.append(C)
    seqs = fc.walks(fam, d, k)
    model = sum(x.walked for x in seqs.values())
    for cache in (True, False):
        if not cache:
            monkeypatch.setenv("CDR_F64_TCACHE", "0")
        for steps in (1, 2, 3):
            C_dev, applied, reason, means, counts = ctx.lloyd_f64_run(c["C"], steps, -1.0)
            assert (applied, reason) == (steps, ctx.F64_RUN_ALL)
            _equal_bits(C_dev, host[steps - 1])
            _equal_bits(means, host[0])  # the same sums and counts in every step
            np.testing.assert_array_equal(ctx.labels(), c["labels"])
            np.testing.assert_array_equal(counts, np.bincount(c["labels"], minlength=k))
            walked = ctx.f64_walked()
            print("\n%s d=%d k=%d cache %s, %d steps: walked blocks device %d, model %d" % (
                fam, d, k, cache, steps, walked, model))
            assert walked > 0
            if fam == "pinned_run":
                assert walked <= model + len(seqs), (walked, model)
            else:
                assert walked <= 2 * model, (walked, model)
        if not cache:
            monkeypatch.delenv("CDR_F64_TCACHE")


def _bounds(n, W):
    """Shard boundaries off every multiple of 256."""
    cut = [0] + [r * n // W + 37 * r for r in range(1, W)] + [n]
    assert all(b % 256 for b in cut[1:-1])
    return cut


@pytest.mark.parametrize("fam,W,force", [
    (fam, W, False) for fam in ("pinned_ties", "growing_ties", "landings", "signs", "signs_prog")
    for W in (2, 3)] + [("growing_ties", 3, True)],
    ids=lambda v: {True: "chain", False: "program"}.get(v, str(v)))
def test_sharded_programs(ctx, monkeypatch, fam, W, force):
    """The sharded programs (f64s_program / f64s_compose) on W contexts with
    ragged shard boundaries: sums and counts = the single context's = NumPy's.
    On the non-negative families the program path itself has to give the
    result (status 0), also on signs_prog with its negative addends, zeros and
    -0.0; signs overflows a program and takes the chain; the forced chain gives
    the same sums."""
    import _cdr

    d, k = 5, 20
    c = fc.case(fam, d, k)
    X, C = c["X"], c["C"]
    if force:
        monkeypatch.setenv("CDR_F64S_FORCE_CHAIN", "1")
    ctx.load_points(X)
    want_s, want_c = ctx.lloyd_step_f64(C)
    labels = ctx.labels()
    _equal_bits(want_s, c["sums"])
    np.testing.assert_array_equal(want_c, np.bincount(c["labels"], minlength=k))
    cut = _bounds(X.shape[0], W)
    ctxs = [_cdr.Context(ctx.device) for _ in range(W)]
    try:
        for r, sh in enumerate(ctxs):
            sh.load_points(X[cut[r]:cut[r + 1]])
            assert sh.info()["mode"] == 2
        outs = _f64_shards_step(ctxs, C)
        print("\nsharded %s W=%d%s: status %s" % (fam, W, " forced chain" if force else "",
                                                 [o[2] for o in outs]))
        for sums, counts, status in outs:
            if force:
                assert status == 1
            elif fam == "signs":
                # sequence 2 never has a binade (negative throughout), so every
                # member of it in a later shard is an ELEM item: ~n / (k W), far
                # beyond the 127 items a program holds, and the chain takes over
                assert status == 1, status
            else:  # the programs themselves give the result: non-negative data, and
                # signs_prog, whose flagged and crossing blocks fit a program as ELEM
                # items (at most 80 items in f64prog_model.shard_program, the CPU test)
                assert status == 0, status
            np.testing.assert_array_equal(counts, want_c)
            _equal_bits(sums, want_s)
        np.testing.assert_array_equal(np.concatenate([sh.labels() for sh in ctxs]), labels)
    finally:
        for sh in ctxs:
            sh.close()


@pytest.mark.parametrize("name", sorted(fc.F32_CASES))
def test_f32r_step_both_storage_modes(ctx, monkeypatch, name):
    """f64_walk<float>: sums_parallel<float, float> (F32X storage) and
    sums_parallel<float, double> against float32 np.add.reduce, the walked
    blocks bounded as for the fp64 instance, and the serial kernel."""
    n, d, k, mode = fc.F32_CASES[name]
    c = fc.case(name, d, k)
    X, C = c["X"], c["C"]
    assert X.dtype == np.float32
    ctx.load_points(X)
    assert ctx.info()["mode"] == mode
    sums, counts = ctx.lloyd_step_f32r(C)
    walked = ctx.f64_walked()
    labels = ctx.labels()
    np.testing.assert_array_equal(labels, ko.assign(X, C))
    np.testing.assert_array_equal(labels, c["labels"])
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=k))
    want = fc.numpy_sums(X, labels, k)
    assert want.dtype == np.float32
    _equal_bits(sums, want.astype(np.float64))
    _check_walked(name, d, k, walked)
    monkeypatch.setenv("CDR_F64_SERIAL", "1")
    s2, c2 = ctx.lloyd_step_f32r(C)
    monkeypatch.delenv("CDR_F64_SERIAL")
    assert ctx.f64_walked() == -1
    _equal_bits(s2, sums)
    np.testing.assert_array_equal(c2, counts)

"""The large-k Lloyd step (csrc/screen_big.hip) at every form its host code
picks, on the designed cases of tests/big_cases.py: all labels and the
(k, d+1) int64 sums equal the oracle's, with no tolerance.  Every case first
asserts through Context.big_layout() that the form it names ran (the expected
values come from big_cases.form, the formulas written out in Python) and that
the levels it targets saw points.

What each assertion would catch:

* form matrix, labels: a ``jkeep`` one bit short maps winners at j >= 2048
  onto j - 2048 (the 2047|2048 ties at k = 2200 / 2300, 4095|4096 at k = 4200);
  a tie broken by the key's low bits instead of the index fails the "half"
  pairs in one of their two orders; a merge of the lane halves or of two
  blocks that prefers the later one fails "halves" / "blocks" / the edges; a
  padded last block read as real centroids fails the winner at k - 1; an
  fp16-only decision fails every near tie; a candidate list that drops the
  16th or keeps a 17th fails the 16- and 17-clusters; an L2 / L3 that takes
  the last of equal roots fails the duplicates;
* ``l2_form``: the (64, 1100), (40, 1500), (20, 2200), (12, 4200) and the two
  limit shapes run cand_big (fragments from global memory), the others
  cand_big_lds; leftovers > 0 and l3 > 0 show L2 and L3 had points;
* delta steps: a move list that loses a region, a fixup that subtracts from
  the wrong row or skips a feature pass of FG = 8 / 4 gives sums that differ
  from the oracle's and from a fresh context's full update_big pass; mv1 > 0
  (a solo cluster swapped), mv2 > 0 (the eviction pairs in L2, the
  17-cluster's location in L3) show the lists were used;
* invalidation: running sums kept across another k or another path would
  give delta = 1 and the sums of the wrong labels;
* device plan: big_plan_kernel against build_plan_big byte for byte;
* many groups: a wrong prefetch or stride in L1's second iteration mislabels
  the points past the first regions * 64;
* limits: the first unsupported k must fail cleanly and leave the context
  usable.

The second many-groups case (d = 17, k = 1500 at n = 393,293, the 768-thread
form) is left out: its oracle takes about two minutes on the CPU.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import big_cases as bc
from oracle import kmeans_oracle as ko
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx2():
    import _cdr

    c = _cdr.Context(0)
    yield c
    c.close()


def _check_form(ctx, d, k, delta, plan=0):
    lay = ctx.big_layout()
    want = bc.form(d, k)
    for key in ("DQ", "KB", "FG", "JB", "l1_threads", "l2_form"):
        assert lay[key] == want[key], (key, lay, want)
    assert lay["delta"] == delta and lay["plan"] == plan, lay
    assert ctx.profile_kernel() == "screen_big_sp<%d,%d>" % (want["DQ"], want["l1_threads"])
    if not delta:
        assert lay["mv1"] == 0 and lay["mv2"] == 0, lay
    return lay


def _step(ctx, X, C, want_labels):
    import _cdr

    out = ctx.lloyd_step(C)
    assert ctx.info()["mode"] == _cdr.MODE_F32X
    np.testing.assert_array_equal(ctx.labels(), want_labels)
    want = bc.sums(X, want_labels, C.shape[0], ctx.info()["scale_bits"])
    np.testing.assert_array_equal(out, want)
    return out


@pytest.mark.parametrize("d,k", list(bc.SHAPES))
def test_form_matrix_and_host_plan_delta(ctx, ctx2, d, k):
    """(a) one step from a fresh load in the form the matrix names, then (b)
    the three delta steps of big_cases.sequence on the host plan; every delta
    step's sums also equal a fresh context's full update pass."""
    X, C, ex = bc.case(d, k)
    steps = bc.sequence(d, k)
    n2 = int((ex["levels"] >= 2).sum())
    n3 = int((ex["levels"] == 3).sum())
    ctx.load_points(X)
    assert ctx.big_layout() == dict.fromkeys(ctx.big_layout(), 0)
    ctx2.load_points(X)
    for t, (Ct, lab) in enumerate(steps):
        out = _step(ctx, X, Ct, lab)
        lay = _check_form(ctx, d, k, 1 if t else 0)
        print(d, k, t, lay)
        if t in (0, 2):   # the designed geometry; the means steps shift it
            assert lay["leftovers"] >= n2 and lay["l3"] >= n3 > 0, (lay, n2, n3)
        assert lay["leftovers"] >= lay["l3"] > 0, lay
        if t == 0:
            np.testing.assert_array_equal(lab[ex["rows"]], ex["labels"])
        else:
            prev = steps[t - 1][1]
            assert lay["mv1"] + lay["mv2"] == int((prev != lab).sum()), lay
            assert lay["mv2"] > 0, lay
            if t == 2:
                assert lay["mv1"] > 0, lay
            ctx2.load_points(X)
            np.testing.assert_array_equal(ctx2.lloyd_step(Ct), out)
            assert ctx2.big_layout()["delta"] == 0


def test_delta_invalidation(ctx):
    """(c) the running sums of one k survive neither another k nor another path."""
    n, d = 5000, 24
    X = synth.generate(n, 0, n, d, 300, 2424)
    ctx.load_points(X)
    rng = np.random.default_rng(24)
    want_delta = [(300, 0), (1200, 0), (300, 0), (300, 1), (33, None), (300, 0)]
    for k, delta in want_delta:
        C = X[np.sort(rng.choice(n, k, replace=False))]
        out = ctx.lloyd_step(C)
        lab, want = ko.lloyd_partials(X, C, ctx.info()["scale_bits"])
        np.testing.assert_array_equal(ctx.labels(), lab)
        np.testing.assert_array_equal(out, want)
        if delta is None:
            # the small-k screen of screen_mid.hip (screen_kernel<2> at this shape; its
            # step (mid_step), shared with screen_fast, drops the large-k running sums)
            assert ctx.profile_kernel().startswith(("screen_kernel", "screen_fast"))
        else:
            _check_form(ctx, d, k, delta)


@pytest.mark.parametrize("d,k", [(40, 1500), (12, 4200), (9, 2300)])
def test_device_plan_loop(ctx, d, k):
    """(d) four steps of the device loop (big_plan_kernel, thr_dev, gate,
    fixup_big<8> and <4>) against ko.lloyd.  The loop is advanced one step at
    a time, as _loop does in chunks, so that the layout of every step can be
    read: each runs on the device plan, and a step is a delta step unless the
    step before it left an empty cluster to the host (which ends the running
    sums); at least one delta step must have run."""
    from cdr_dist import DeviceLloyd

    X, C0, _ = bc.case(d, k, False)
    ctx.load_points(X)
    np.random.seed(5)
    run = DeviceLloyd(ctx, np.array(C0), -1.0, lambda g: X[g], X.shape[0])
    lays = []
    try:
        for _ in range(4):
            assert run.advance(1) == 1
            lays.append(_check_form(ctx, d, k, ctx.big_layout()["delta"], plan=1))
    except BaseException:
        ctx.lloyd_end()
        raise
    C, st = run.finish()
    np.random.seed(5)
    Cr, empties = np.array(C0), []
    for _ in range(4):
        lab_ref = ko.assign(X, Cr)
        empties.append(bool((np.bincount(lab_ref, minlength=k) == 0).any()))
        Cr = ko.update(X, lab_ref, Cr, X.shape[0])
    assert st["steps"] == 4
    np.testing.assert_array_equal(ctx.labels(), lab_ref)
    np.testing.assert_array_equal(C, Cr)
    print(d, k, empties, [(l["delta"], l["mv1"], l["mv2"]) for l in lays])
    assert [l["delta"] for l in lays] == [0] + [0 if e else 1 for e in empties[:3]]
    assert any(l["delta"] and l["mv1"] + l["mv2"] > 0 for l in lays), lays
    assert all(l["leftovers"] > 0 for l in lays), lays


@pytest.mark.parametrize("d,k", [(40, 1500), (12, 4200), (9, 2300), (64, 1100)])
def test_plan_parity_host_and_device(ctx, d, k):
    """The host plan (build_plan_big) and the device plan (big_plan_kernel) of
    the same centroids are the same bytes, thresholds included."""
    from cdr_dist import DeviceLloyd

    X, C, _ = bc.case(d, k)
    lab = bc.sequence(d, k)[0][1]
    ctx.load_points(X)
    ctx.lloyd_step(C)
    _check_form(ctx, d, k, 0, plan=0)
    host = ctx.debug_big_plan(k)
    run = DeviceLloyd(ctx, np.array(C), -1.0, lambda g: X[g], X.shape[0])
    try:
        ctx.lloyd_enqueue_assign(None)   # one step on the device plan of C
        _check_form(ctx, d, k, 0, plan=1)
        dev = ctx.debug_big_plan(k)
        np.testing.assert_array_equal(ctx.labels(), lab)
    finally:
        ctx.lloyd_end()
    np.testing.assert_array_equal(dev["C"], C)
    for key in ("frag1", "cinit", "C"):
        np.testing.assert_array_equal(host[key], dev[key], err_msg=key)
    assert host["thr"].tolist() == dev["thr"].tolist(), (host["thr"], dev["thr"])
    assert host["thr"][0] > 0 and host["thr"][1] == np.float32(1.0 + 2.0 ** (bc.form(d, k)["JB"] - 21))


def _assign_rows(X, C, parts=16):
    """ko.assign over row chunks in threads (the rows are independent)."""
    cuts = np.linspace(0, X.shape[0], parts + 1).astype(int)
    with ThreadPoolExecutor(parts) as ex:
        labs = list(ex.map(lambda i: ko.assign(X[cuts[i]:cuts[i + 1]], C), range(parts)))
    return np.concatenate(labs)


def test_many_groups_per_wave(ctx):
    """(e) more 64-point groups than L1 waves: the prefetch-and-stride loop of
    screen_big_sp runs a second time (d = 33, k = 257: DQ 3, 8 waves a
    workgroup), in a fresh and in a delta step."""
    import torch

    d, k = 33, 257
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = bc.form(d, k)["l1_threads"] // 64
    n = 2 * (cus * waves * 64) + 77
    X = np.floor(synth.generate(n, 0, n, d, k, 3357) * 1024.0) / 1024.0
    rng = np.random.default_rng(33)
    C = X[np.sort(rng.choice(n, k, replace=False))]
    ctx.load_points(X)
    for t in range(2):
        lab = _assign_rows(X, C)
        _step(ctx, X, C, lab)
        lay = _check_form(ctx, d, k, t)
        assert lay["regions"] == cus * waves and lay["groups"] > 2 * lay["regions"], lay
        if t:
            assert lay["mv1"] + lay["mv2"] == int((lab != prev).sum()) > 0
        prev, C = lab, bc.means(X, lab, C)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_tiny_and_ragged_n(ctx, n):
    """(f) fewer points than one workgroup's waves: most regions are empty."""
    d, k = 64, 1100
    X, C, ex = bc.case(d, k)
    rows = np.concatenate([ex["rows"], np.setdiff1d(np.arange(X.shape[0]), ex["rows"])])[:n]
    Xs = np.ascontiguousarray(X[rows[::-1]])
    ctx.load_points(Xs)
    for t in range(2):
        lab = ko.assign(Xs, C)
        _step(ctx, Xs, C, lab)
        lay = _check_form(ctx, d, k, t)
        assert lay["groups"] == -(-n // 64), lay
        C = bc.means(Xs, lab, C)


@pytest.mark.parametrize("d,k", [(64, 1152), (12, 4256)])
def test_limits(ctx, d, k):
    """(g) the first unsupported k raises and leaves the context usable; the
    last supported one then runs a full step."""
    X, C, _ = bc.case(d, k)
    lab = bc.sequence(d, k)[0][1]
    ctx.load_points(X)
    _step(ctx, X, C, lab)
    C_over = np.concatenate([C, X[:1]])
    assert not bc.form(d, k + 1)["supported"]
    with pytest.raises(NotImplementedError, match="too large for the update table"):
        ctx.lloyd_step(C_over)
    _step(ctx, X, C, lab)
    _check_form(ctx, d, k, 0)


def test_small_d_is_not_supported(ctx):
    X = synth.generate(4000, 0, 4000, 7, 16, 7)
    ctx.load_points(X)
    with pytest.raises(NotImplementedError, match="too large for the update table"):
        ctx.lloyd_step(X[:3000])

"""The watch list of the 2-byte bounded screen (screen32bs16's WATCH form,
DESIGN.md 4.3h) at small sizes: CDR_S32BS_WATCH_MIN=1 switches the list path
on below its size threshold and CDR_S32BS_CUS=8 gives 128 waves, so a wave's
range is a few 512-point chunks and its region one to four 16-byte loads.

A point that is not listed is not looked at while the list is streamed, so a
wrong budget threshold, a stale entry or a list kept across a reset shows as
a label the oracle does not give.  Every step is checked: labels against the
oracle's assignment from the previous centroids and the centroids against
X[labels == j].mean(axis=0), bit for bit (src/kmeans_plusplus.py:33-41), with
the list on and off.  Each case asserts through Context.watch_info() that the
path it is about ran (list steps, full steps, builds)."""
import functools

import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from oracle import synth
from test_gpu_screen_layout import _check_every_step, _data, _reference, _switches

pytestmark = pytest.mark.gpu

STEPS = 14
# d = 16, k = 64: 256 chunks, two per wave; d = 8, k = 16: 128 chunks, one per wave
SHAPES = {16: (131_072 - 71, 16, 64), 8: (65_536 - 4_533, 8, 16)}
_ref = functools.lru_cache(maxsize=6)(_reference)
# Uniform and mirrored points at these sizes fail most of their words every
# step, so their lists pass the default capacity (half a wave's range); with
# room for the whole range they are listed all the same, and hundreds of
# entries of a wave fail at once (the LDS list fills and is compacted).
WHOLE = 65_536


def _watch(monkeypatch, on=True, beta=None, cap=None):
    _switches(monkeypatch, cus=8)
    monkeypatch.setenv("CDR_S32BS_WATCH", "1" if on else "0")
    monkeypatch.setenv("CDR_S32BS_WATCH_MIN", "1")
    for name, v in (("CDR_S32BS_WATCH_BETA", beta), ("CDR_S32BS_WATCH_CAP", cap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _steps(ctx, X, C0, steps, each=None):
    """`steps` device-loop steps enqueued one at a time: the labels and
    centroids after each and the watch list's state (each(info): a further
    check after every step)."""
    from cdr_dist import DeviceLloyd

    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, np.array(C0, dtype=np.float64), -1.0, lambda g: X[g], X.shape[0])
    out, infos = [], []
    try:
        for _ in range(steps):
            assert run.advance(1) == 1
            out.append((ctx.labels(), ctx.lloyd_read()[0]))
            infos.append(ctx.watch_info())
            if each is not None:
                each(infos[-1])
    finally:
        ctx.lloyd_end()
    print("\nmodes", [i["mode"] for i in infos], "listed", [i["listed"] for i in infos],
          "failed", [i["failed"] for i in infos], "epochs", infos[-1]["epochs"])
    return out, infos


@pytest.mark.parametrize("kind,dd", [("blobs", 16), ("uniform", 16), ("mirror", 16),
                                     ("blobs", 8), ("uniform", 8), ("mirror", 8)])
def test_list_on_and_off_equal_the_oracle_every_step(ctx, monkeypatch, kind, dd):
    """Parity: 14 steps with the list on and with it off."""
    n, d, k = SHAPES[dd]
    X, C0, traj = _ref(kind, n, d, k, STEPS)
    _watch(monkeypatch, cap=None if (kind, dd) == ("blobs", 16) else WHOLE)
    got, infos = _steps(ctx, X, C0, STEPS)
    _check_every_step(got, traj)
    # the first build slot with words to list follows step 5
    assert infos[-1]["list_steps"] >= 4 and infos[-1]["epochs"] >= 1, infos[-1]
    # ((blobs, 16) at the default capacity: 24 % of the points are listed then)
    assert all(i["mode"] == 0 for i in infos[2:5]) and infos[5]["mode"] == 1, infos
    # a list step tests its entries only
    assert all(i["failed"] <= i["listed"] for i in infos if i["mode"] == 1), infos
    _watch(monkeypatch, on=False)
    off, infos_off = _steps(ctx, X, C0, STEPS)
    assert all(i["mode"] == -1 for i in infos_off), infos_off
    _check_every_step(off, got)


def _invariant(ctx, n):
    """The list after a step, against the words: every entry's word is its
    point's, and no real point outside the list could fail before the budget
    is spent."""
    def check(info):
        if not info["next_list"]:
            return
        w = ctx.debug_watch()
        words, rng_, cnt = w["words"], w["range"], w["counts"]
        assert np.all(w["T"] <= w["HL"]), (w["T"], w["HL"])
        listed = np.zeros(words.size, dtype=bool)
        for wave in range(w["waves"]):
            ent = w["entries"][wave, :cnt[wave]]
            pts = wave * rng_ + (ent >> 16).astype(np.int64)
            assert np.unique(pts).size == pts.size
            np.testing.assert_array_equal(ent & 0xFFFF, words[pts])
            listed[pts] = True
        rest = words[:n][~listed[:n]]
        assert np.all((rest >> 6) > w["HL"][rest & 63]), "an unlisted point within the budget"
        assert not listed[n:].any(), "a padding row is listed"
        check.done += 1
    check.done = 0
    return check


@pytest.mark.parametrize("kind,dd", [("uniform", 16), ("mirror", 8)])
def test_unlisted_points_are_outside_the_budget(ctx, monkeypatch, kind, dd):
    """Invariant: after every step the list stands, read back."""
    n, d, k = SHAPES[dd]
    X, C0, traj = _ref(kind, n, d, k, STEPS)
    _watch(monkeypatch, cap=WHOLE)
    check = _invariant(ctx, X.shape[0])
    got, infos = _steps(ctx, X, C0, STEPS, each=check)
    _check_every_step(got, traj)
    assert check.done >= 6, check.done


def test_overflow_streams_every_word(ctx, monkeypatch):
    """A budget that lists almost every point into regions of 256 entries
    (1024 points per wave): the build overflows, every step streams the
    words, and no build is tried again except with a rebase (new codes)."""
    n, d, k = SHAPES[16]
    X, C0, traj = _ref("uniform", n, d, k, STEPS)
    _watch(monkeypatch, beta=1000, cap=256)
    got, infos = _steps(ctx, X, C0, STEPS)
    _check_every_step(got, traj)
    last = infos[-1]
    assert last["cap"] == 256 and last["list_steps"] == 0, last
    assert 1 <= last["epochs"] <= last["carried"] + 1, last
    assert last["full_steps"] == STEPS - 1, last  # (step 1 is the full screen)


def test_budget_spent_inside_an_epoch(ctx, monkeypatch):
    """beta = 1/64: the thresholds pass the budget before the next build
    slot, so list steps, then full steps up to the slot, then list steps
    again."""
    n, d, k = SHAPES[16]
    X, C0, traj = _ref("uniform", n, d, k, STEPS)
    _watch(monkeypatch, beta=0.015625, cap=WHOLE)
    check = _invariant(ctx, X.shape[0])
    got, infos = _steps(ctx, X, C0, STEPS, each=check)
    _check_every_step(got, traj)
    modes = [i["mode"] for i in infos[5:]]
    s = "".join(str(m) for m in modes)
    assert "10" in s and "01" in s[s.index("10"):], modes
    assert infos[-1]["epochs"] >= 2


def test_rebase_rebuilds_a_standing_list(ctx, monkeypatch):
    """A rebase inside the run: the words carried to the new base and
    listed in one pass, the list steps before and after it equal to the
    oracle's."""
    n, d, k = SHAPES[8]
    steps = 22
    X, C0, traj = _ref("blobs", n, d, k, steps)
    _watch(monkeypatch, beta=64, cap=WHOLE)
    got, infos = _steps(ctx, X, C0, steps, each=_invariant(ctx, X.shape[0]))
    _check_every_step(got, traj)
    # (the first build, after step 5, carries nothing: the words were reset)
    assert infos[-1]["carried"] >= 1 and infos[-1]["list_steps"] >= 8, infos[-1]


def _list_peak(f, absolute):
    """The highest LDS list index the WATCH form's phase 1 reaches for a wave
    whose 256-entry loads hold f[i] failing entries: the index logic of
    screen32bs.hip (groups of 4 loads, step2 between them gathering 64 entries
    and compacting when head > 0 and cnt + 256 > 640).  absolute: the room
    before an insert counted from cnt, as the kernel does; else from head, the
    guard that let a dense block behind sparse failures write past the list."""
    LS, room = 640, 256
    cnt = head = g0 = peak = 0
    first = True
    while True:
        more = g0 < len(f)
        if not first:
            last = not more
            while True:
                pend, avail = False, cnt - head
                if avail >= 64 or (last and avail > 0):
                    head += min(avail, 64)
                    pend = True
                if head > 0 and not last and cnt + room > LS:
                    cnt, head = cnt - head, 0
                if not ((pend or cnt > head) if last else (cnt - head + room > LS)):
                    break
        first = False
        if not more:
            return peak
        adv = 0
        for i in range(4):
            if g0 + i >= len(f) or (cnt if absolute else cnt - head) + room > LS:
                break
            cnt += int(f[g0 + i])
            peak = max(peak, cnt)
            adv = i + 1
        g0 += adv


def test_dense_block_behind_sparse_failures_stays_inside_the_lds_list(ctx, monkeypatch):
    """28 loads per wave (7,168 points, all listed: beta = 1000, whole-range
    regions).  In nine waves every 16th point sits at the centre of mirrored
    blobs (a near tie with every mirrored pair: it keeps no usable bound and
    fails every step), so a group of four loads adds about 64 failures and
    step2 gathers 64: cnt and head climb together, without a compaction, to
    ~384.  Then 1,024 such points in a row, at a different place in each of
    the nine waves: loads that fail entirely.  The list holds 640 entries and
    the slots start right behind them, so room counted from head would let
    the block write to index 896.  _list_peak replays the kernel's index logic
    on the entries read back before each list step: the input reaches the
    case (the old guard's peak passes 640) and the kernel's guard stays
    inside; labels and centroids equal the oracle's at every step."""
    from cdr_dist import DeviceLloyd

    d, k, rng_pts, waves = 8, 16, 7168, 128
    n = waves * rng_pts - 300
    h = synth.generate(n // 2, 0, n // 2, d, k // 2, 77)
    X = np.concatenate([h, 1.0 - h])
    rs = np.random.default_rng(78)
    rows = []
    for w in range(9):
        r = np.arange(rng_pts)
        blk = (r >= 512 * (4 + w)) & (r < 512 * (6 + w))
        rows.append(w * rng_pts + r[blk | (r % 16 == 0)])
    rows = np.concatenate(rows)
    X[rows] = 0.5 + np.ldexp(rs.integers(-3, 4, (rows.size, d)).astype(np.float64), -24)
    half = X[70_000 + rs.choice(n // 2 - 70_000, k // 2, replace=False)]
    C0 = np.concatenate([half, 1.0 - half])
    _watch(monkeypatch, beta=1000, cap=WHOLE)
    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, C0.copy(), -1.0, lambda g: X[g], n)
    got, infos, old_peak, new_peak = [], [], 0, 0
    try:
        for s in range(STEPS):
            assert run.advance(1) == 1
            got.append((ctx.labels(), ctx.lloyd_read()[0]))
            infos.append(ctx.watch_info())
            if infos[-1]["next_list"]:  # what the next screen will stream and test
                w = ctx.debug_watch()
                assert (w["range"], w["waves"]) == (rng_pts, waves), infos[-1]
                for wave in range(9):
                    ent = w["entries"][wave, :w["counts"][wave]]
                    fail = ((ent >> 6) & 1023) <= w["T"][ent & 63]
                    f = np.add.reduceat(fail.astype(np.int64), np.arange(0, ent.size, 256))
                    old_peak = max(old_peak, _list_peak(f, False))
                    new_peak = max(new_peak, _list_peak(f, True))
    finally:
        ctx.lloyd_end()
    print("\nmodes", [i["mode"] for i in infos], "failed", [i["failed"] for i in infos],
          "peaks", old_peak, new_peak)
    np.random.seed(3)
    C, traj = C0.copy(), []
    for _ in range(STEPS):
        lab = ko.assign(X, C)
        C = ko.update(X, lab, C, n)
        traj.append((lab, C))
    _check_every_step(got, traj)
    assert infos[-1]["list_steps"] >= 6, infos[-1]
    assert new_peak <= 640 < old_peak, (old_peak, new_peak)


def test_resume_and_take_over_drop_a_standing_list(ctx, monkeypatch):
    """After step 9, while the screens stream a list, cdr_lloyd_resume with
    other centroids (one of them far away); that centroid's cluster is empty
    in the next step, so the loop stops and the host takes over (reseed,
    resume).  Neither may leave the list standing: the words are reset, so an
    entry of the old list is stale.  No screen streams a list until a new one
    has been built, and every step equals the oracle's."""
    from cdr_dist import DeviceLloyd

    n, d, k = SHAPES[8]
    X, C0 = _data("blobs", n, d, k)
    steps, at, far = 22, 9, 5
    _watch(monkeypatch, cap=WHOLE)
    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, np.array(C0, dtype=np.float64), -1.0, lambda g: X[g], n)
    got, infos, stops = [], [], []
    try:
        for s in range(steps):
            if s == at:
                assert infos[-1]["mode"] == 1 and infos[-1]["next_list"] == 1, infos[-1]
                C_new = ctx.lloyd_read()[0].copy()
                C_new[far] = 5.0
                ctx.lloyd_resume(C_new, 0)
            assert run.advance(1) == 1
            stops.append(run.status["reason"])
            got.append((ctx.labels(), ctx.lloyd_read()[0]))
            infos.append(ctx.watch_info())
    finally:
        ctx.lloyd_end()
    print("\nmodes", [i["mode"] for i in infos], "list_steps", [i["list_steps"] for i in infos],
          "epochs", [i["epochs"] for i in infos], "stops", stops)
    assert stops[at] == ctx.LL_EMPTY and stops.count(ctx.LL_EMPTY) == 1, stops  # the take-over
    np.random.seed(3)
    C, traj = np.array(C0, dtype=np.float64), []
    for s in range(steps):
        if s == at:
            C = C.copy()
            C[far] = 5.0
        lab = ko.assign(X, C)
        C = ko.update(X, lab, C, n)
        traj.append((lab, C))
    _check_every_step(got, traj)
    # from the resume on, a screen streams a list only after a later build
    e0, l0 = infos[at - 1]["epochs"], infos[at - 1]["list_steps"]
    for s in range(at, steps):
        if infos[s]["list_steps"] > infos[s - 1]["list_steps"]:
            assert infos[s - 1]["epochs"] > e0, (s, infos[s - 1], infos[s])
    assert infos[-1]["epochs"] > e0 and infos[-1]["list_steps"] > l0, infos[-1]
    # the first bounded screen after the take-over finds every word reset
    first = next(s for s in range(at, steps) if infos[s]["full_steps"] > infos[at - 1]["full_steps"])
    assert infos[first]["mode"] == 0 and infos[first]["failed"] == n, infos[first]


def test_two_sharded_contexts_equal_one(monkeypatch):
    """Two contexts with a summed buffer between assign and finalize (the
    multi-GPU step): each keeps its own list; the result is the oracle's."""
    import torch

    import _cdr

    n, d, k = SHAPES[16]
    X, C0, traj = _ref("uniform", n, d, k, STEPS)
    _watch(monkeypatch, cap=WHOLE)
    cut = 57_344
    ctxs = [_cdr.Context(0), _cdr.Context(0)]
    try:
        ctxs[0].load_points(X[:cut])
        ctxs[1].load_points(X[cut:])
        # one transform on both shards (cdr_dist.unify_points)
        sts = [c.points_stats() for c in ctxs]
        dd = (sts[0].size - 3) // 2
        g = np.concatenate([np.minimum(sts[0][:dd], sts[1][:dd]),
                            np.maximum(sts[0][dd:], sts[1][dd:])])
        for c in ctxs:
            c.points_restat(g, n)
        ref = C0[0].copy()
        x2 = sum(c.points_sqdev(ref) for c in ctxs)
        bufs = [torch.zeros(k * (d + 1), dtype=torch.int64, device="cuda") for _ in ctxs]
        for c in ctxs:
            c.lloyd_begin(np.array(C0), -1.0, ref, x2)
        for s in range(STEPS):
            for c, b in zip(ctxs, bufs):
                c.lloyd_enqueue_assign(b.data_ptr())
            for c in ctxs:
                c.synchronize()
            tot = bufs[0] + bufs[1]
            for b in bufs:
                b.copy_(tot)
            torch.cuda.synchronize()
            for c, b in zip(ctxs, bufs):
                c.lloyd_enqueue_finalize(b.data_ptr())
            labs = np.concatenate([c.labels() for c in ctxs])
            np.testing.assert_array_equal(labs, traj[s][0], err_msg=f"labels of step {s + 1}")
            for c in ctxs:
                np.testing.assert_array_equal(c.lloyd_read()[0], traj[s][1])
        infos = [c.watch_info() for c in ctxs]
        for c in ctxs:
            c.lloyd_end()
    finally:
        for c in ctxs:
            c.close()
    assert all(i["list_steps"] >= 4 for i in infos), infos

"""The list path's one launch per step (screen32bsw): the
kernel reads the mode word once and runs the default or the WATCH body; the
WATCH body issues the list's count and first four entry loads with the plan's
loads, before it knows the count, and its tail records carry the point's
offset and the entry's slot as two 16-bit halves.

The switches and read-backs are those of test_gpu_watch_list.py
(CDR_S32BS_WATCH_MIN=1 and CDR_S32BS_CUS=8: the list path at small sizes, 128
waves; CDR_S32BS_WATCH_CAP, CDR_S32BS_WATCH_BETA; Context.watch_info() and
debug_watch()).  Every step is checked against the oracle bit for bit: a list
entry tested against a stale count, a load past a wave's region or a record
unpacked with a sign shows as a label the oracle does not give."""
import numpy as np
import pytest

from oracle import kmeans_oracle as ko
from oracle import synth
from test_gpu_screen_layout import _check_every_step
from test_gpu_watch_list import SHAPES, STEPS, WHOLE, _ref, _steps, _watch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,dd,k", [("blobs", 16, 64), ("uniform", 16, 64), ("blobs", 8, 16),
                                       ("uniform", 8, 16), ("uniform", 16, 32)])
def test_every_step_runs_exactly_one_form(ctx, monkeypatch, kind, dd, k):
    """131,001 x 16, k = 64 and 61,003 x 8, k = 16, 14 steps: each bounded
    step counts as a FULL or a LIST step, never as both or neither, both kinds
    occur, and the step reports the name screen32bs16<Q,MT>.  k = 32 at d = 16
    is <4,1>, the one shape that keeps a launch per form (each gated on the
    mode word) instead of the one kernel running either.  CDR_S32BS_WATCH=0:
    the same results from the default form's own kernel, and no list counter
    moves."""
    n, d, _ = SHAPES[dd]
    X, C0, traj = _ref(kind, n, d, k, STEPS)
    name = "screen32bs16<%d,%d>" % (d // 4, 1 if k <= 32 else 2)
    _watch(monkeypatch, cap=None if (kind, dd) == ("blobs", 16) else WHOLE)
    seen = []

    def each(info):
        seen.append((info["full_steps"], info["list_steps"], ctx.profile_kernel()))

    got, infos = _steps(ctx, X, C0, STEPS, each=each)
    _check_every_step(got, traj)
    # a bounded step is one that reports the bounded screen (the first step,
    # and the step that rebuilds the bounds, run the full screen32 pass)
    bounded, before = 0, 0
    for s, (full, lst, kern) in enumerate(seen):
        if kern.startswith("screen32bs"):
            assert kern == name, (s, kern)
            bounded += 1
        assert full + lst == bounded and full + lst - before in (0, 1), (s, seen)
        before = full + lst
    full, lst, _ = seen[-1]
    assert bounded >= STEPS - 3 and full > 0 and lst > 0, seen
    _watch(monkeypatch, on=False)
    seen.clear()
    off, infos_off = _steps(ctx, X, C0, STEPS, each=each)
    _check_every_step(off, got)
    assert all(i["mode"] == -1 and i["listed"] == 0 and i["failed"] == 0 for i in infos_off), infos_off
    assert all((f, l) == (0, 0) for f, l, _ in seen), seen
    assert sum(kern == name for _, _, kern in seen) == bounded, seen


# ---- the hoisted loads at the edges of a list ----
E_D, E_K, E_RANGE, E_WAVES, E_STEPS = 8, 16, 2048, 128, 10
E_N = E_WAVES * E_RANGE - 300
# the rows of uniform points at the start of each wave's range: by the wave's
# index modulo 4, with one row in wave 9; E_BIG: more than half a range
E_QUIET = 4  # tight blobs, one start centroid each
E_BASE = (0, 150, 100, 37)
E_BIG = {3: 1500, 60: 1333, 127: 1100}  # (wave 127: the region that ends the buffer)


def _edges_data(blocks):
    """Most rows are points of four tight blobs in corners of the cube, far
    from everything else: their centroids stand still, their bounds never come
    near the budget, and a wave that holds nothing else lists nothing.  The
    first rows of a wave's range are uniform points of the opposite corner
    region (E_BASE, `blocks` {wave: rows} over it), which twelve centroids
    share: they keep moving for the test's steps and nearly all of them are
    listed at the first build."""
    rs = np.random.default_rng(4243)
    corners = np.array([[0.9] * 8, [0.9, 0.1] * 4, [0.1, 0.9] * 4, [0.9] * 4 + [0.6] * 4])
    corners = np.round(np.ldexp(corners, 24)) / 16777216.0  # (the 2^-24 grid: exact in fp32)
    X = corners[rs.integers(0, E_QUIET, E_N)] + np.ldexp(
        rs.integers(-1024, 1025, (E_N, E_D)).astype(np.float64), -24)
    rows = []
    for wave in range(E_WAVES):
        m = blocks.get(wave, 1 if wave == 9 else E_BASE[wave % 4])
        m = min(m, E_N - wave * E_RANGE)
        rows.append(wave * E_RANGE + np.arange(m))
    rows = np.concatenate(rows)
    X[rows] = np.ldexp(rs.integers(1 << 20, 7 << 20, (rows.size, E_D)).astype(np.float64), -24)
    C0 = np.concatenate([corners, X[np.sort(rs.choice(rows, E_K - E_QUIET, replace=False))]])
    return X, C0


def _list_checks(ctx, n, seen):
    """Before each list step: the per-wave counts the screen will stream
    (collected in `seen`), and the list's invariants against the words -
    (1) every entry carries its point's word, (2) no point is listed twice and
    no padding row is listed, (3) every real point outside the list is above
    the budget's threshold of its label."""
    def check(info):
        if not info["next_list"]:
            return
        w = ctx.debug_watch()
        words, rng_, cnt = w["words"], w["range"], w["counts"]
        assert np.all(w["T"] <= w["HL"]), (w["T"], w["HL"])
        assert np.all(cnt >= 0) and np.all(cnt <= w["cap"]), cnt
        listed = np.zeros(words.size, dtype=bool)
        for wave in range(w["waves"]):
            ent = w["entries"][wave, :cnt[wave]]
            off = (ent >> 16).astype(np.int64)
            assert np.all(off < rng_)
            pts = wave * rng_ + off
            assert np.unique(pts).size == pts.size, wave
            np.testing.assert_array_equal(ent & 0xFFFF, words[pts])
            listed[pts] = True
        assert not listed[n:].any(), "a padding row is listed"
        rest = words[:n][~listed[:n]]
        assert np.all((rest >> 6) > w["HL"][rest & 63]), "an unlisted point within the budget"
        seen.append(cnt.copy())
    return check


def _oracle_steps(X, C0, steps):
    np.random.seed(3)
    C, traj = np.array(C0, dtype=np.float64), []
    for _ in range(steps):
        lab = ko.assign(X, C)
        C = ko.update(X, lab, C, X.shape[0])
        traj.append((lab, C))
    return traj


@pytest.mark.parametrize("cap,blocks", [(WHOLE, E_BIG), (256, {})],
                         ids=["whole-range", "one-load"])
def test_hoisted_loads_at_the_edges_of_a_list(ctx, monkeypatch, cap, blocks):
    """128 waves of 2,048 points, 10 steps (the first list follows step 5).
    The first group's four loads go out before the count is known, clamped to
    the region: list steps must stream a wave
    with no entry (four loads of stale entries, none tested), waves with
    1..255 entries (one load, the rest behind the count), and - regions of a
    whole range - waves with more than 1,024 entries and a ragged last load
    (groups after the first), one of them the last wave, whose region ends the
    buffer.  Regions of 256 entries: the four loads are the region's one load.
    The counts read back before each list step show that each case ran."""
    X, C0 = _edges_data(blocks)
    traj = _oracle_steps(X, C0, E_STEPS)
    _watch(monkeypatch, cap=cap)
    seen = []
    got, infos = _steps(ctx, X, C0, E_STEPS, each=_list_checks(ctx, E_N, seen))
    _check_every_step(got, traj)
    last = infos[-1]
    assert (last["range"], last["waves"]) == (E_RANGE, E_WAVES), last
    assert last["cap"] == min(cap, E_RANGE) and last["list_steps"] >= 4, last
    # the counts of the list steps that ran: every read-back but one taken
    # after the last step is followed by a LIST step
    ran = np.array(seen[:-1] if infos[-1]["next_list"] else seen)
    print("list steps read back", len(ran), "empty waves", int((ran == 0).sum()),
          "1..255", int(((ran >= 1) & (ran <= 255)).sum()), "max", int(ran.max()))
    assert len(ran) >= 4
    assert (ran == 0).any(), "no wave without entries"
    assert ((ran >= 1) & (ran <= 255)).any(), "no wave with 1..255 entries"
    if cap == WHOLE:
        big = ran[(ran > 1024) & (ran % 256 != 0)]
        assert big.size > 0, "no wave with more than 1,024 entries and a ragged last load"
        assert (ran[:, E_WAVES - 1] > 1024).any(), "the last wave's list is short"
    else:
        assert ran.max() <= 256


# ---- tail records at the 16-bit limits ----
T_N, T_D, T_K = 8_388_608, 8, 16  # 128 waves x 65,536 points
T_RANGE, T_WAVES, T_STEPS = 65_536, 128, 6


def _assign_ties(X, C, chunk=1 << 20):
    """ko.assign's loop (the first index of the smallest root) keeping the
    runner-up too: the labels and the rows whose two smallest roots are equal."""
    labels = np.empty(X.shape[0], dtype=np.int64)
    tied = np.zeros(X.shape[0], dtype=bool)
    for s in range(0, X.shape[0], chunk):
        Xs = X[s:s + chunk]
        best = np.full(Xs.shape[0], np.inf)
        second = np.full(Xs.shape[0], np.inf)
        lab = np.zeros(Xs.shape[0], dtype=np.int64)
        for j in range(C.shape[0]):
            r = np.sqrt(ko.sqdist_rows(Xs, C[j]))
            better = r < best
            second = np.where(better, best, np.minimum(second, r))
            best = np.where(better, r, best)
            lab[better] = j
        labels[s:s + chunk] = lab
        tied[s:s + chunk] = best == second
    return labels, np.flatnonzero(tied)


T_TIE_WAVES, T_TIES = (0, 64, T_WAVES - 1), 2048  # tied rows: the last 2,048 of these ranges
G = 1.0 / 16777216.0  # the data's grid


def _balanced(rs, count, width):
    """count x width offsets of up to 1,024 grid steps whose every column
    sums to zero (count even): a set built on them has its centre as mean."""
    k = rs.integers(0, 1025, (count // 2, width)).astype(np.float64)
    return np.concatenate([k, -k]) * G


def _limits_data():
    """Seven blobs with two start centroids each, and in a corner of the cube,
    far from every blob, two clusters of their own whose centroids stand still
    from the start and keep exact ties at every step (mirror symmetry cannot:
    a tied point goes to the lower index, so the pair's counts differ after
    the first update).  Cluster 0 is 6,144 rows A around x0 = 1/256 and the
    6,144 tied rows T at x0 = 1/256 + 1/16 exactly; cluster 1 is 6,144 rows B
    around x0 = 1/256 + 3/32; every other feature is 1/256 with offsets that
    sum to zero in each set.  All sums are exact, so the means are
    c0 = 1/256 + 1/32 and c1 = 1/256 + 3/32 in x0 and 1/256 elsewhere, bit for
    bit, at every step: a row of T is 1/32 from both in x0 and equally far in
    the rest, and the first index, 0, takes it.  T is the last 2,048 rows of
    three waves' ranges (offsets 63,488 and up), A and B stand before it.
    Returns X, C0, the oracle's (labels, centroids) of every step, the
    exactly tied rows of every step and T's rows."""
    X = synth.generate(T_N, 0, T_N, T_D, 7, 515)
    sample = X[70_000:270_000]
    idx = [0]
    dmin = ((sample - sample[0]) ** 2).sum(axis=1)
    for _ in range(1, T_K - 2):
        idx.append(int(np.argmax(dmin)))
        dmin = np.minimum(dmin, ((sample - sample[idx[-1]]) ** 2).sum(axis=1))
    rs = np.random.default_rng(516)
    w, pa = 1.0 / 256, 1.0 / 256
    t, c0, c1 = pa + 1.0 / 16, pa + 1.0 / 32, pa + 3.0 / 32
    m = T_TIES * len(T_TIE_WAVES)
    ends = np.array([(wv + 1) * T_RANGE for wv in T_TIE_WAVES])
    rows_t = np.concatenate([np.arange(e - T_TIES, e) for e in ends])
    rows_a = np.concatenate([np.arange(e - 2 * T_TIES, e - T_TIES) for e in ends])
    rows_b = np.concatenate([np.arange(e - 3 * T_TIES, e - 2 * T_TIES) for e in ends])
    for rows, x0, spread in ((rows_a, pa, True), (rows_t, t, False), (rows_b, c1, True)):
        X[rows] = w + _balanced(rs, m, T_D)
        X[rows, 0] = x0 + (_balanced(rs, m, 1)[:, 0] if spread else 0.0)
    C0 = np.concatenate([np.full((2, T_D), w), sample[np.array(idx)]])
    C0[0, 0], C0[1, 0] = c0, c1
    np.random.seed(3)
    C, traj, ties = C0.copy(), [], []
    for _ in range(T_STEPS):
        lab, tied = _assign_ties(X, C)
        C = ko.update(X, lab, C, T_N)
        traj.append((lab, C))
        ties.append(tied)
    return X, C0, traj, ties, rows_t


def test_tail_records_at_the_16_bit_limits(ctx, monkeypatch):
    """8,388,608 x 8, k = 16 on the 8-CU grid: 128 waves whose range is
    exactly 65,536 points, regions of a whole range and beta = 1024, so nearly
    every point is listed and slots reach the top of the region; 6 steps, the
    last of them a LIST step (the first build slot follows step 5).  6,144
    rows tie exactly between centroids 0 and 1 at every step (_limits_data), at
    offsets of 63,488 and more of three ranges; they keep no bound, so they
    are listed, fail in the LIST step and leave near-tie records there, whose
    offset and slot are both 32,768 or more: unpacked with a sign they would
    name other points.  Labels and centroids equal the oracle's at every step;
    the oracle's tied rows of every step are those rows, and the fallback
    count of every bounded step, the LIST step among them, is at least their
    number (a point that nearly ties takes the same pass), as
    test_gpu_screen_mid_dispatch.py checks it.  The oracle's six assignments
    of 8.4M points are most of the test's time."""
    from cdr_dist import DeviceLloyd

    X, C0, traj, ties, rows_t = _limits_data()
    for s, tied in enumerate(ties):
        assert tied.size >= rows_t.size and np.isin(rows_t, tied).all(), (s, tied.size)
        assert (rows_t % T_RANGE >= T_RANGE - T_TIES).all()
        assert (traj[s][0][rows_t] == 0).all()
        np.testing.assert_array_equal(traj[s][1][:2], C0[:2])
    _watch(monkeypatch, beta=1024, cap=T_RANGE)
    ctx.load_points(X)
    np.random.seed(3)
    run = DeviceLloyd(ctx, C0.copy(), -1.0, lambda g: X[g], T_N)
    got, infos, fallbacks, slots = [], [], [], None
    try:
        for s in range(T_STEPS):
            assert run.advance(1) == 1
            fallbacks.append(ctx.fallback_count())
            got.append((ctx.labels(), ctx.lloyd_read()[0]))
            infos.append(ctx.watch_info())
            if s == T_STEPS - 2:  # the list the last step streams: the tied rows' slots
                assert infos[-1]["next_list"] == 1, infos[-1]
                w = ctx.debug_watch()
                slots = []
                for wv in T_TIE_WAVES:
                    off = w["entries"][wv, :w["counts"][wv]] >> 16
                    slots.append(np.flatnonzero(off >= T_RANGE - T_TIES))
    finally:
        ctx.lloyd_end()
    print("modes", [i["mode"] for i in infos], "failed", [i["failed"] for i in infos],
          "fallbacks", fallbacks, "ties", [t.size for t in ties],
          "lowest slot of a tied row", min(int(sl.min()) for sl in slots))
    _check_every_step(got, traj)
    last = infos[-1]
    assert (last["range"], last["cap"], last["waves"]) == (T_RANGE, T_RANGE, T_WAVES), last
    assert last["mode"] == 1 and last["list_steps"] == 1, infos
    # every tied row is listed, in a slot of the region's upper half
    assert all(sl.size == T_TIES and sl.min() >= T_RANGE // 2 for sl in slots), slots
    assert last["failed"] >= rows_t.size
    for s in range(1, T_STEPS):  # (step 1 is the full screen32 pass)
        assert fallbacks[s] >= ties[s].size > 0, (s, fallbacks, [t.size for t in ties])

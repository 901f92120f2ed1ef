"""The event case builders (tests/event_cases.py) have the properties the GPU
tests rely on: each sort-fallback log takes the route, pass count, tile count
and span it is named for (from the restated host logic); the stability log
loses its concurrency when a file's events are reordered; the exchange logs
hold every listed client and op; the width logs have a local event through a
primary of at least 2^30 and a READ in a bucket of each kernel's shape; the K6
tables have their edge.  No GPU."""
import numpy as np
import pytest

import event_cases as ec
from oracle import features_oracle as fo


def _route(name):
    f, op, cl, ts, prim = ec.sort_case(name)
    return ec.sort_route(f, ts, prim.size), (f, op, cl, ts, prim)


@pytest.mark.parametrize("nf,passes", zip(ec.R32_NF, (1, 2, 2, 3)))
def test_k32_pass_counts(nf, passes):
    r, (f, *_r, prim) = _route("r32-nf%d" % nf)
    assert (r["kind"], r["passes"], prim.size) == ("k32", passes, nf)
    assert (f == nf - 1).any() and (f == -1).any() and (f >= nf).any()


@pytest.mark.parametrize("shape,passes", zip(ec.R64, ec.R64_PASSES))
def test_k64_pass_counts(shape, passes):
    r, (f, op, cl, ts, prim) = _route("r64-p%d" % passes)
    assert (r["kind"], r["passes"], prim.size) == ("k64", passes, shape[0])
    assert r["span"] == shape[1] - 1 and (ts == ec.NULL).any()
    if passes == 7:
        assert r["sbits"] == 32 and r["end_bit"] == 53 and ts[ts != ec.NULL].min() < 0
    # the hand-written group-by would take these logs, so they need the switch
    # (but for the last: its hash key of 10 + 32 bits is over 40)
    assert (ec.hand_layout(f, cl, ts, prim.size) is None) == (passes == 7)


@pytest.mark.parametrize("n", ec.TILE_N + (ec.SCAN_N,))
def test_tile_and_scan_sizes(n):
    for kind, name in (("k32", "n32-%d" % n), ("k64", "n64-%d" % n)):
        if n == ec.SCAN_N:
            name = "scan" + kind[1:]
        r, (f, *_r) = _route(name)
        assert (r["kind"], f.size, r["unsorted"]) == (kind, n, True), name
        assert r["tiles"] == -(-n // ec.RS_TILE)
    if n == ec.SCAN_N:
        assert r["tiles"] == 258 > ec.RS_CHUNK  # rs_scan carries into a second loop turn


def test_same_digit_logs():
    r, (f, *_r) = _route("digit64")
    assert r["kind"] == "k64" and r["passes"] == 4 and np.unique(f).size == 1
    for p in (2, 3):
        assert np.unique((r["keys"] >> np.uint64(8 * p)) & np.uint64(255)).size == 1
    r, _ = _route("digit32")
    assert r["kind"] == "k32" and r["passes"] == 3
    assert np.unique(r["keys"] & np.uint64(255)).size == 1


def test_invalid_only_logs():
    for name, kind in (("invalid32", "k32"), ("invalid64", "k64")):
        r, (f, *_r, prim) = _route(name)
        assert r["kind"] == kind and not ((f >= 0) & (f < prim.size)).any()
        assert (f == -1).any() and (f >= prim.size).any()


def test_stability_log_discriminates():
    r, (f, op, cl, ts, prim) = _route("stable")
    nf = prim.size
    assert r["kind"] == "k32" and r["unsorted"] and r["tiles"] == 2
    exp = fo.counts_from_arrays(f, op, cl, ts, prim, nf)[0][:, 5]
    stable = np.argsort(np.where((f >= 0) & (f < nf), f, nf), kind="stable")
    np.testing.assert_array_equal(ec.run_concurrency(f, ts, nf, stable), exp)
    for hot, B in ec.STABLE_HOT.items():
        pos = np.flatnonzero(f == hot)
        assert pos.min() < B <= pos.max() and B % 64 == 0
        sec = ts[pos] // ec.US
        cnt = np.bincount(sec - sec.min())
        assert cnt.tolist() == [3, 4, 3] and exp[hot] == 4  # consecutive seconds, >= 3 each
        # the four events of the middle second lie on both sides of B
        mid = pos[sec == sec.min() + 1]
        assert (mid < B).sum() == 2 and (mid >= B).sum() == 2
        got = ec.run_concurrency(f, ts, nf, ec.unstable_order(f, nf, hot, B))
        assert got[hot] == 3 and (got != exp).sum() == 1
    Bs = sorted(ec.STABLE_HOT.values())
    assert Bs[0] % ec.RS_CHUNK and Bs[1] % ec.RS_CHUNK == 0 and Bs[1] % ec.RS_TILE
    assert Bs[2] == ec.RS_TILE


def test_per_file32_spans():
    r, (f, *_r, prim) = _route("perfile32")
    assert r["kind"] == "k32" and r["unsorted"] and prim.size == ec.PF_NF and ec.PF_NF % 64
    spans = ec.group_spans(f, ec.PF_NF)
    assert spans[:3].tolist() == [ec.PER_FILE_STAGE, ec.PER_FILE_STAGE + 1, 0]
    g3 = f[(f >= 192) & (f < 256)]
    assert g3.size > 0 and np.unique(g3).size == 1
    assert 0 < spans[4] <= ec.PER_FILE_STAGE and (f == -1).any() and (f >= ec.PF_NF).any()


def test_shortcut_logs():
    for name, kind in (("sorted32", "k32"), ("sorted64", "k64"), ("pair", "k32"), ("one", "k64")):
        r, (f, op, cl, ts, prim) = _route(name)
        assert (r["kind"], r["unsorted"], r["passes"]) == (kind, False, 0), name
    assert (ec.sort_case("sorted64")[3] == ec.NULL).any()
    assert (ec.sort_case("sorted32")[0] >= 700).any()
    assert ec.sort_case("pair")[0].size == 2 and ec.sort_case("one")[0].size == 1


def test_nulls_at_32_second_bits():
    r, (f, op, cl, ts, prim) = _route("nulls32bit")
    assert r["kind"] == "k64" and r["sbits"] == 32 and r["unsorted"]
    assert (ts[f == 0] == ec.NULL).all() and (f == 0).sum() > 1
    t1 = ts[f == 1]
    assert (t1 == ec.NULL).any() and (t1 != ec.NULL).any()
    assert set((ts[f == 2] // ec.US).tolist()) == {-1, -2}
    exp = fo.counts_from_arrays(f, op, cl, ts, prim, 6)[0]
    assert exp[0, 5] == 7 and exp[1, 5] == 5 and exp[2, 5] == 3 and exp[5, 0] == 0


def test_natural_entries_are_declined_by_the_payload_width():
    f, op, cl, ts, prim = ec.sort_case("natural64")
    assert prim.size == 4 and ec.second_range(ts) == 1 << 31 and cl.max() == ec.WIDE_CLIENT
    assert ec.hand_layout(f, cl, ts, 4) is None
    narrow = np.minimum(cl, 3)  # one bit fewer and the hand-written path takes it
    assert ec.hand_layout(f, narrow, ts, 4)["pbits"] < 64
    r = ec.sort_route(f, ts, 4)
    assert (r["kind"], r["sbits"], r["unsorted"]) == ("k64", 32, True) and (ts == ec.NULL).any()
    assert fo.counts_from_arrays(f, op, cl, ts, prim, 4)[0][2, 3] >= 1  # local by the wide id

    f, op, cl, ts, prim = ec.sort_case("natural32")
    assert prim.size == 1100 and ec.second_range(ts) == (1 << 29) - 1
    assert ec.hand_layout(f, cl, ts, 1100) is None
    lay = ec.hand_layout(f, np.minimum(cl, (1 << 30) - 2), ts, 1100)
    assert lay["pbits"] == 64 and lay["sbits"] == 30 and lay["cbits"] == 30
    r = ec.sort_route(f, ts, 1100)
    assert (r["kind"], r["ordered"], r["passes"]) == ("k32", True, 2)
    top = ts // ec.US - ts.min() // ec.US == (1 << 29) - 1
    assert (f[top] == 1099).sum() == 3  # the top second value, three times in one file
    assert fo.counts_from_arrays(f, op, cl, ts, prim, 1100)[0][1099, 5] >= 3

    f, op, cl, ts, prim = ec.sort_case("refused")
    assert ec.second_range(ts) == 1 << 32 and ec.hand_layout(f, cl, ts, 4) is None
    assert ec.sort_route(f, ts, 4)["refused"]

    for name, kind in (("nomanifest-ordered", "k32"), ("nomanifest-shuffled", "k64")):
        f, op, cl, ts, prim = ec.sort_case(name)
        assert prim.size == 0 and f.size == 1000 and ec.hand_layout(f, cl, ts, 0) is None
        assert ec.sort_route(f, ts, 0)["kind"] == kind
    ts = ec.sort_case("nomanifest-shuffled")[3]
    assert ts[-1] != ts[ts != ec.NULL].max() and (ts == ec.NULL).any()


@pytest.mark.parametrize("kernel", list(ec.WIDTH_SHAPES))
@pytest.mark.parametrize("cmax", ec.WIDTH_CMAX)
def test_width_logs(kernel, cmax):
    f, op, cl, ts, prim = ec.width_log(kernel, cmax)
    ne, nf, span, switch = ec.WIDTH_SHAPES[kernel]
    assert 20_000 <= f.size == ne <= 200_000 and cl.max() == cmax
    lay = ec.hand_layout(f, cl, ts, nf)
    assert lay["cbits"] == {0: 30, 1: 31, 2: 31, 3: 31, 4: 32}[ec.WIDTH_CMAX.index(cmax)]
    assert lay["payload_bytes"] == 8
    first = ec.bucket_kernel(lay, {switch} if switch else ())
    valid = (f >= 0) & (f < nf)
    per_bucket = np.bincount(f[valid] >> lay["L"], minlength=-(-nf // (1 << lay["L"])))
    cap = ec.GB_DENSE_CAP if lay["dense"] else ec.GB_LDS_CAP
    over = per_bucket > cap
    reads = np.bincount(f[valid & (op == 2)] >> lay["L"], minlength=per_bucket.size) > 0
    if kernel == "gb_bucket_big":
        assert first == "gb_bucket" and (over & reads).any()
    else:
        assert first == kernel and not over.any() and reads.any()
    assert {0, 1, 2} <= set(np.unique(op).tolist())
    local = valid & (cl >= 0) & (cl == prim[np.where(valid, f, 0)])
    assert local.sum() >= 2000
    wide = min(cmax, 1 << 30)
    assert (local & (cl >= wide)).sum() >= 1 and (prim >= 1 << 30).any()
    assert local[0] and cl[0] == cmax and op[0] == 2  # a local READ by the widest id


@pytest.mark.parametrize("ne", ec.X_NE)
def test_exchange_logs(ne):
    f, op, cl, ts, prim = ec.exchange_log(ne)
    assert f.size == ne and prim.size == ec.X_NF
    assert not ((f >= ec.X_HOLE[0]) & (f < ec.X_HOLE[1])).any()
    if ne >= 255:
        assert set(ec.X_CLIENTS) <= set(cl.tolist()) and set(op.tolist()) == {0, 1, 2}
        assert (f == -1).any() and (f >= ec.X_NF).any() and (ts == ec.NULL).any()
        assert -ec.X_CLIENT_LIM in cl and cl.max() == ec.X_CLIENT_LIM - 1
    assert (ec.exchange_log(257, "all")[3] == ec.NULL).all()
    assert ec.X_NE[-1] > ec.FIN_THREADS  # x_pack's outer loop takes a second turn


@pytest.mark.parametrize("nr", [1, 2, 257, 1024])
def test_exchange_bounds(nr):
    f, op, cl, ts, prim = ec.exchange_log(70_001)
    for kind in ("even", "runs", "window", "hole"):
        b = ec.exchange_bounds(kind, nr)
        assert b.size == nr + 1 and (np.diff(b) >= 0).all() and b[0] >= 0 and b[-1] <= ec.X_NF
        counts, rec, mx = ec.exchange_expect(f, op, cl, ts, b)
        assert mx == ts[ts != ec.NULL].max()
        if kind == "hole":
            assert counts.sum() == 0
        if kind == "window":
            assert b[0] > 0 and b[-1] < ec.X_NF and 0 < counts.sum() < ((f >= 0) & (f < ec.X_NF)).sum()
        if kind in ("runs", "window") and nr > 2:
            assert (np.diff(b) == 0).sum() >= nr // 2  # runs of empty owners
        # the records say what was sent: decode them again
        assert rec.size == 0 or (rec["cop"] >> 8).min() >= -ec.X_CLIENT_LIM
        own = np.repeat(np.arange(nr), counts)
        assert ((rec["file"] >= b[own]) & (rec["file"] < b[own + 1])).all()


@pytest.mark.parametrize("name", ec.FIN_CASES)
def test_fin_cases(name):
    c, cr, obs = ec.fin_case(name)
    t = fo.finalize(c, cr, obs)
    assert np.isfinite(t).all()
    if name == "one":
        assert c.shape[0] == 1 and not t[0, 5:].any()
    elif name == "constant":
        assert not t[:, 5:].any()
    elif name == "nowrites":
        assert not c[:, 1].any() and not t[:, 2].any()  # mean 0 -> 1.0, ratio 0 / 1
    elif name == "total0":
        assert (c[::3, 4] == 0).all() and (t[::3, 3] == 1.0).all()
        assert (t[1::3, 3] == 0.0).all() and (t[2::3, 3] == 1.0).all()
    elif name == "allnan":
        assert np.isnan(cr).all() and not t[:, 1].any() and not t[:, 6].any()
    elif name == "future":
        assert (t[:, 1] < 0).any() and (t[:, 1] > 0).any()
    elif name == "lastbit":
        ages = np.unique(t[:, 1])
        assert ages.size == 3 and np.nextafter(ages[0], np.inf) == ages[1]
    elif name == "two53":
        # the difference to the minimum is only exact when taken in integers
        af = c[:, 0]
        naive = (af.astype(np.float64) - float(af.min())) / float(af.max() - af.min())
        assert (naive != t[:, 5]).any() and af.min() > 1 << 52
    elif name == "grid":
        assert c.shape[0] == ec.FIN_THREADS + 3

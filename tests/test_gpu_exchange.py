"""The exchange record of csrc/exchange.hip on one context: pack (x_count,
x_pack) against NumPy, unpack (x_unpack) read back with features_events_read
and aggregated against the oracle, and the 24-bit client field's range check.
tests/event_cases.py builds the logs and bounds (tests/test_event_cases.py
shows that they hold every listed client, op and bound shape)."""
import numpy as np
import pytest

import event_cases as ec
from oracle import features_oracle as fo

pytestmark = pytest.mark.gpu
NULL = ec.NULL


def _pack(ctx, log, bounds):
    f, op, cl, ts, prim = log
    ctx.features_load_events(f, op, cl, ts, prim)
    send, counts, mx = ctx.features_exchange_pack(bounds)
    ecounts, erec, emx = ec.exchange_expect(f, op, cl, ts, bounds)
    np.testing.assert_array_equal(counts, ecounts)
    assert mx == emx
    got = ec.sort_records(send, counts)
    np.testing.assert_array_equal(got, erec)
    return send, counts, mx


@pytest.mark.parametrize("ne", ec.X_NE)
def test_pack_event_counts(ctx, ne):
    """0 events to one more than a launch holds (x_pack's outer loop turns
    twice), 257 owners with runs of empty ones inside a window of the
    manifest: events outside the window are not sent but enter the maximum."""
    _pack(ctx, ec.exchange_log(ne), ec.exchange_bounds("window", 257))


@pytest.mark.parametrize("kind", ["even", "runs", "window", "hole"])
@pytest.mark.parametrize("nr", [1, 2, 257, 1024])
def test_pack_ranks_and_bounds(ctx, nr, kind):
    send, counts, _ = _pack(ctx, ec.exchange_log(70_001), ec.exchange_bounds(kind, nr))
    assert (counts.sum() == 0) == (kind == "hole")


def test_pack_nothing_to_send_takes_no_buffer(ctx):
    """A window no event falls in: the C call takes a null send pointer."""
    import ctypes

    f, op, cl, ts, prim = ec.exchange_log(70_001)
    ctx.features_load_events(f, op, cl, ts, prim)
    bounds = ec.exchange_bounds("hole", 2)
    counts = np.full(2, -1, dtype=np.int64)
    mx = ctypes.c_int64(0)
    rc = ctx._lib.cdr_features_exchange_pack(ctx._h, 2, bounds.ctypes.data, None,
                                             counts.ctypes.data, ctypes.byref(mx))
    assert rc == 0 and not counts.any() and mx.value == ts[ts != NULL].max()


def test_pack_all_null_timestamps(ctx):
    _, counts, mx = _pack(ctx, ec.exchange_log(257, "all"), ec.exchange_bounds("even", 2))
    assert mx == -2 ** 63 and counts.sum() > 0


def test_pack_over_1024_ranks_raises(ctx):
    ctx.features_load_events(*ec.exchange_log(257))
    with pytest.raises(ValueError, match="1..1024 ranks"):
        ctx.features_exchange_pack(ec.exchange_bounds("even", 1025))


UNPACK_BOUNDS = np.array([50, 50, ec.X_HOLE[0], ec.X_HOLE[1], 2500, 4000], dtype=np.int64)


@pytest.mark.parametrize("owner", [1, 2, 4])
def test_unpack_gives_the_owner_its_events(ctx, owner):
    """Owner 1: file_begin > 0 with records; owner 2: a range with zero
    records; owner 4: the last range, short of the manifest's end.  (Owner 0's range is empty: see
    test_unpack_empty_range.)"""
    f, op, cl, ts, prim = log = ec.exchange_log(70_001)
    send, counts, _ = _pack(ctx, log, UNPACK_BOUNDS)
    off = np.concatenate([[0], np.cumsum(counts)])
    rec = np.frombuffer(send.tobytes(), dtype=ec.XREC)[off[owner]:off[owner + 1]]
    lo, hi = int(UNPACK_BOUNDS[owner]), int(UNPACK_BOUNDS[owner + 1])
    assert lo > 0 and (rec.size == 0) == (owner == 2)
    ctx.features_exchange_unpack(rec.view(np.uint8).copy(), rec.size, lo, hi)
    gf, gop, gcl, gts, gpr = ctx.features_events_read()
    # the records' own fields, in their order; clients exact, negatives included
    np.testing.assert_array_equal(gf, rec["file"] - lo)
    np.testing.assert_array_equal(gcl, rec["cop"] >> 8)
    np.testing.assert_array_equal(gop, rec["cop"] & 0xFF)
    np.testing.assert_array_equal(gts, rec["ts"])
    np.testing.assert_array_equal(gpr, prim[lo:hi])
    mine = (f >= lo) & (f < hi)
    np.testing.assert_array_equal(np.sort(gcl), np.sort(cl[mine]))
    got, mx = ctx.features_aggregate_resident()
    exp, emx = fo.counts_from_arrays(f[mine] - lo, op[mine], cl[mine], ts[mine], prim[lo:hi],
                                     hi - lo)
    np.testing.assert_array_equal(got, exp)
    assert mx == (NULL if emx is None else emx)
    if owner != 2:
        assert (gcl < 0).any() and got[:, 3].sum() > 0


def test_unpack_empty_range(ctx):
    """An owner without rows receives nothing and holds no events after."""
    ctx.features_load_events(*ec.exchange_log(257))
    ctx.features_exchange_unpack(np.zeros(16, dtype=np.uint8), 0, 50, 50)
    assert ctx._ev == (0, 0)
    with pytest.raises(RuntimeError, match="no resident events"):
        ctx.features_aggregate_resident()


def test_unpack_widens_the_client_field_to_the_received_ids(ctx):
    """The context held clients up to 3; the records carry 2^23 - 1: the
    group-by's payload must grow to hold them (8 bytes here, 4 before)."""
    f, op, cl, ts, prim = ec.exchange_log(70_001)
    prim = prim.copy()
    prim[::7] = ec.X_CLIENT_LIM - 1
    ctx.features_load_events(f, op, cl, ts, prim)
    bounds = np.array([0, 2048], dtype=np.int64)
    send, counts, _ = ctx.features_exchange_pack(bounds)
    n = int(counts[0])
    narrow = np.clip(cl, -3, 3)
    ctx.features_load_events(f, op, narrow, ts, prim)
    ctx.features_aggregate_resident()
    assert ctx.features_groupby_info()["payload_bytes"] == 4
    ctx.features_exchange_unpack(send[:16 * n].copy(), n, 0, 2048)
    got, _ = ctx.features_aggregate_resident()
    info = ctx.features_groupby_info()
    mine = (f >= 0) & (f < 2048)
    exp, _ = fo.counts_from_arrays(f[mine], op[mine], cl[mine], ts[mine], prim[:2048], 2048)
    np.testing.assert_array_equal(got, exp)
    assert info["hand"] == 1 and info["payload_bytes"] == 8, info
    assert (cl[mine] == prim[f[mine]])[cl[mine] == ec.X_CLIENT_LIM - 1].sum() > 0


@pytest.mark.parametrize("client,ok", [(ec.X_CLIENT_LIM - 1, True), (ec.X_CLIENT_LIM, False),
                                       (-ec.X_CLIENT_LIM, True), (-ec.X_CLIENT_LIM - 1, False),
                                       (2 ** 31 - 1, False), (-2 ** 31, False)])
def test_pack_refuses_a_client_outside_24_bits(ctx, client, ok):
    """The record holds the client as a signed 24-bit value: the last values
    it holds round-trip, the next ones raise instead of being cut."""
    f, op, cl, ts, prim = ec.exchange_log(257)
    f, cl = f.copy(), np.clip(cl, -3, 3)
    f[200], cl[200] = 1234, client
    bounds = ec.exchange_bounds("even", 2)
    ctx.features_load_events(f, op, cl, ts, prim)
    if not ok:
        with pytest.raises(NotImplementedError, match="2\\^23"):
            ctx.features_exchange_pack(bounds)
        return
    send, counts, _ = ctx.features_exchange_pack(bounds)
    rec = np.frombuffer(send[:16 * int(counts.sum())].tobytes(), dtype=ec.XREC)
    assert (rec["cop"][rec["file"] == 1234] >> 8).tolist().count(client) == 1
    ctx.features_exchange_unpack(send[:16 * int(counts[0])].copy(), int(counts[0]), 0,
                                 int(bounds[1]))
    assert client in ctx.features_events_read()[2]

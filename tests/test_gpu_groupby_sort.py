"""The group-by's sort fallback (csrc/features.hip's sort-based path over the
stable LSD radix sort of csrc/radix.hip) on its own routes, against the
oracle's independent group-by (oracle/features_oracle.counts_from_arrays).

Natural entries run with no switch: logs groupby_resident declines (a payload
over 64 bits on either key type, an empty manifest) and a span the fallback
refuses.  The shapes of the route's kernels run under CDR_GROUPBY_SORT=1:
every radix pass count from 1 to 7 and both final buffers, the tile and scan
edges of rs_hist / rs_scan / rs_scatter, stability across lane, chunk and tile
boundaries, per_file32's staged and global-memory spans, the already-sorted
shortcuts, and nulls at 32 second bits.  tests/event_cases.py builds the logs
and tests/test_event_cases.py proves on the CPU that each has the property it
is named for.  An 8-pass sort needs 2^24 manifest files (a 100 MiB table per
call) and is left out.

The first assertion of every test is that the fallback ran."""
import numpy as np
import pytest

import event_cases as ec

pytestmark = pytest.mark.gpu


def _run(ctx, name, entry):
    """The case's counts through either entry call, and what ran."""
    f, op, cl, ts, prim = ec.sort_case(name)
    if entry == "upload":
        got, mx = ctx.features_aggregate(f, op, cl, ts, prim)
    else:
        ctx.features_load_events(f, op, cl, ts, prim)
        got, mx = ctx.features_aggregate_resident()
    return got, mx, ctx.features_groupby_info()


def _check(ctx, name, entry):
    got, mx, info = _run(ctx, name, entry)
    assert info["hand"] == 0, info
    exp, emx = ec.sort_expect(name)
    np.testing.assert_array_equal(got, exp)
    assert mx == emx
    return got


# ---- natural entries: no environment variable --------------------------------
@pytest.mark.parametrize("entry", ["upload", "resident"])
@pytest.mark.parametrize("name", ["natural64", "natural32"])
def test_payload_over_64_bits_takes_the_fallback(ctx, name, entry):
    got = _check(ctx, name, entry)
    assert got[:, 3].sum() > 0


@pytest.mark.parametrize("name", ["nomanifest-ordered", "nomanifest-shuffled"])
def test_empty_manifest_with_events(ctx, name):
    got = _check(ctx, name, "upload")
    assert got.shape == (0, 6)


def test_span_over_2_32_seconds_is_refused_and_the_context_lives_on(ctx):
    with pytest.raises(NotImplementedError, match="more than 2\\^32 seconds"):
        _run(ctx, "refused", "upload")
    assert ctx.features_groupby_info()["hand"] == 0
    f, op, cl, ts, prim = ec.sort_case("n64-4097")  # the next, ordinary call
    got, mx = ctx.features_aggregate(f, op, cl, ts, prim)
    exp, emx = ec.sort_expect("n64-4097")
    np.testing.assert_array_equal(got, exp)
    assert mx == emx
    with pytest.raises(NotImplementedError, match="more than 2\\^32 seconds"):
        _run(ctx, "refused", "resident")
    got, mx, _ = _run(ctx, "n32-4097", "resident")
    np.testing.assert_array_equal(got, ec.sort_expect("n32-4097")[0])


# ---- the route's kernels: CDR_GROUPBY_SORT=1 ---------------------------------
@pytest.fixture
def sort_only(monkeypatch):
    monkeypatch.setenv("CDR_GROUPBY_SORT", "1")


PASS_CASES = ["r32-nf%d" % nf for nf in ec.R32_NF] + ["r64-p%d" % p for p in ec.R64_PASSES]


@pytest.mark.parametrize("i,name", list(enumerate(PASS_CASES)))
def test_radix_pass_counts_and_final_buffer(ctx, sort_only, i, name):
    """1, 2, 2, 3 passes of 32-bit keys and 1, 2, 3, 4, 7 of 64-bit keys: an
    even count leaves the result in the first buffer pair."""
    _check(ctx, name, ("upload", "resident")[i % 2])


@pytest.mark.parametrize("n", ec.TILE_N)
@pytest.mark.parametrize("keys", ["32", "64"])
def test_tile_edges(ctx, sort_only, keys, n):
    _check(ctx, "n%s-%d" % (keys, n), ("upload", "resident")[n % 2])


@pytest.mark.parametrize("keys", ["32", "64"])
def test_scan_carry_over_256_tiles(ctx, sort_only, keys):
    """258 tiles: rs_scan's loop takes a second turn and carries the first
    256 tiles' total into it."""
    _check(ctx, "scan" + keys, "resident" if keys == "32" else "upload")


@pytest.mark.parametrize("name", ["digit32", "digit64", "invalid32", "invalid64"])
def test_one_digit_and_invalid_only_logs(ctx, sort_only, name):
    got = _check(ctx, name, "upload")
    assert (got.sum() == 0) == name.startswith("invalid")


def test_sort_is_stable_across_lane_chunk_and_tile_boundaries(ctx, sort_only):
    """max_concurrency on the 32-bit route is a run length in the sorted
    order: it equals the oracle's only if each file's events stay in time
    order."""
    got = _check(ctx, "stable", "upload")
    assert [got[h, 5] for h in ec.STABLE_HOT] == [4, 4, 4]


def test_per_file32_staged_and_global_spans(ctx, sort_only):
    got = _check(ctx, "perfile32", "resident")
    assert got[:64, 0].sum() == ec.PER_FILE_STAGE and got[64:128, 0].sum() == ec.PER_FILE_STAGE + 1
    assert not got[128:192].any()


@pytest.mark.parametrize("name,entry", [("sorted32", "upload"), ("sorted64", "resident"),
                                        ("pair", "resident"), ("one", "upload"),
                                        ("one", "resident")])
def test_already_sorted_shortcuts(ctx, sort_only, name, entry):
    _check(ctx, name, entry)


@pytest.mark.parametrize("entry", ["upload", "resident"])
def test_nulls_at_32_second_bits(ctx, sort_only, entry):
    got = _check(ctx, "nulls32bit", entry)
    assert got[0, 5] == got[0, 0] == 7  # only nulls: one group

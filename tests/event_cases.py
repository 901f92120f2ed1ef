"""Event logs and count tables for the tests of the event paths off the main
group-by route (TEST INFRASTRUCTURE ONLY): the sort fallback of
csrc/features.hip + csrc/radix.hip, wide client ids in the bucket kernels of
csrc/groupby_bucket.hip, the exchange record of csrc/exchange.hip and K6
(fin_reduce / fin_apply).

Every case is named for the property it is there for (a radix pass count, a
tile count, a staged span of exactly 768 values, ...).  ``sort_route`` and
``hand_layout`` restate the host-side choices of features_aggregate_resident
and groupby_resident in NumPy, so tests/test_event_cases.py proves without a
GPU that each case has its property; the GPU tests (test_gpu_groupby_sort.py,
test_gpu_groupby.py, test_gpu_exchange.py, test_gpu_finalize.py) then only
compare against the oracle.

An event log is (file, op, client, ts_us, primary): int32, uint8, int32, int64
(``NULL`` = null timestamp) and int32 of n_files entries.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import features_oracle as fo

NULL = fo.TS_NULL
T0 = 1_700_000_000_000_000
US = 1_000_000

# constants of the kernels the cases are sized by
RS_TILE = 4096        # radix.hip kRsTile: elements per tile
RS_CHUNK = 256        # rs_scatter: elements per chunk; rs_scan: tiles per loop turn
PER_FILE_STAGE = 768  # features.hip kPerFileStage: values a wave stages in LDS
GB_MAX_DIGIT, GB_MAX_L, GB_LDS_CAP = 9, 10, 3072       # groupby.h / groupby_pay.h
GB_DENSE_BITS, GB_DENSE_CAP, GW_MAX_L = 12, 65535, 8
X_CLIENT_LIM = 1 << 23  # exchange.hip: record clients lie in [-2^23, 2^23)
FIN_THREADS = 4096 * 256  # threads of one fin_reduce / fin_apply / x_pack launch


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def seconds(ts):
    """floor(ts / 1e6) of the non-null timestamps (exact for |ts| < 9e15)."""
    return np.floor_divide(ts[ts != NULL], US)


def second_range(ts) -> int:
    s = seconds(ts)
    return int(s.max() - s.min()) if s.size else 0


# ---- the host-side route choices, restated ---------------------------------
def sort_route(f, ts, nf):
    """features_aggregate_resident's sort-based path on this log: which key
    type, how many radix passes (0: the already-sorted shortcut), how many
    tiles; ``refused`` for a span the path cannot hold."""
    ne = f.size
    real = ts != NULL
    ordered = bool(real.all() and (ne < 2 or (np.diff(ts) >= 0).all()))
    span = second_range(ts)
    if span >= (1 << 32) - 1:
        return {"refused": True}
    smin = int(seconds(ts).min()) if real.any() else 0
    sbits = 1
    while (1 << sbits) - 1 <= span:
        sbits += 1
    fbits = 1
    while (1 << fbits) < nf:
        fbits += 1
    fb32 = 1
    while (1 << fb32) <= nf:
        fb32 += 1
    valid = (f >= 0) & (f < nf)
    fv = np.where(valid, f, 0).astype(np.uint64)
    if ne > 1 and ordered and fb32 <= 31 and span < (1 << 29):
        kind, bits = "k32", fb32
        keys = np.where(valid, fv, np.uint64((1 << fb32) - 1))
    else:
        kind, bits = "k64", min(64, sbits + fbits + 1)
        so = np.where(real, np.floor_divide(np.where(real, ts, 0), US) - smin, (1 << sbits) - 1)
        keys = np.where(valid, (fv << np.uint64(sbits)) | so.astype(np.uint64),
                        np.uint64(2 ** 64 - 1))
    unsorted = bool(ne > 1 and (keys[:-1] > keys[1:]).any())
    return {"refused": False, "kind": kind, "ordered": ordered, "span": span, "sbits": sbits,
            "fbits": fbits, "fb32": fb32, "end_bit": bits, "unsorted": unsorted,
            "passes": -(-bits // 8) if unsorted else 0, "tiles": -(-ne // RS_TILE), "keys": keys}


def hand_layout(f, cl, ts, nf):
    """groupby_resident's layout for this log, or None where it declines
    (the caller then takes the sort-based path)."""
    ne = f.size
    if nf < 1 or ne >= 1 << 31:
        return None
    cmax = max(int(cl.max()), 0) if ne else 0
    cbits = max(1, (cmax + 1).bit_length())
    fbits = (nf - 1).bit_length()
    B1 = min(GB_MAX_DIGIT, fbits)
    rem = fbits - B1
    Lmin, Lmax = max(0, rem - GB_MAX_DIGIT), min(rem, GB_MAX_L)
    if Lmin > Lmax:
        return None
    span = second_range(ts)
    if span >= 1 << 40:
        return None
    sbits = max(1, (span + 1).bit_length())
    nvalid = int(((f >= 0) & (f < nf)).sum())
    a = max(nvalid, 1) / nf

    def shape(lmin):
        dn = sbits + lmin <= GB_DENSE_BITS
        if dn:
            return max(lmin, min(math.floor(math.log2(2048.0 / a)), Lmax,
                                 GB_DENSE_BITS - sbits)), dn
        return max(lmin, min(math.floor(math.log2(1024.0 / a)), Lmax)), dn

    L, dense = shape(Lmin)
    B2, B3 = rem - L, 0
    if rem > GB_MAX_DIGIT and a * 2.0 ** L > 0.5 * GB_LDS_CAP:
        L3, dn3 = shape(max(0, rem - 2 * GB_MAX_DIGIT))
        if rem - GB_MAX_DIGIT - L3 >= 1 and L3 < L:
            L, dense, B2, B3 = L3, dn3, GB_MAX_DIGIT, rem - GB_MAX_DIGIT - L3
    if not dense and L + sbits > 40:
        return None
    pbits = 2 + cbits + sbits + (fbits - B1)
    if pbits > 64:
        return None
    return {"L": L, "dense": int(dense), "sbits": sbits, "cbits": cbits, "pbits": pbits,
            "payload_bytes": 4 if pbits <= 32 else 8, "passes": 3 if B3 else (2 if B2 else 1)}


def bucket_kernel(lay, env=()):
    """gb_buckets_t's first kernel for a layout under the given switches."""
    if not lay["dense"]:
        return "gb_bucket"
    if lay["L"] > GW_MAX_L or "CDR_GB_BLOCK" in env:
        return "gb_bucket_dense"
    return "gb_bucket_wave4" if lay["L"] <= 2 and "CDR_GB_BALLOT" not in env else "gb_bucket_wave"


def run_concurrency(f, ts, nf, order):
    """per_file_run's max_concurrency when the events arrive in ``order``: the
    longest run of equal seconds among a file's events as they are laid out.
    It equals the oracle's count per (file, second) only if every file's
    events are in time order, i.e. if the sort by file was stable."""
    out = np.zeros(nf, dtype=np.int64)
    fo_, so = f[order], np.floor_divide(ts[order], US)
    prev_f, prev_s, run = -1, None, 0
    for ff, ss in zip(fo_.tolist(), so.tolist()):
        if ff < 0 or ff >= nf:
            prev_f = -1
            continue
        run = run + 1 if (ff == prev_f and ss == prev_s) else 1
        prev_f, prev_s = ff, ss
        out[ff] = max(out[ff], run)
    return out


# ---- event logs --------------------------------------------------------------
def _fill(rng, f, ts, nf, nclients=4):
    """op, client and primaries for given files and timestamps: every op,
    null and foreign clients, primaries that are no node, many local events."""
    ne = f.size
    op = rng.integers(0, 3, ne).astype(np.uint8)
    cl = rng.integers(-1, nclients, ne).astype(np.int32)
    cl[rng.random(ne) < 0.02] = -3
    prim = rng.integers(-2, nclients, nf).astype(np.int32)
    return _ro(f.astype(np.int32), op, cl, ts.astype(np.int64), prim)


def _ordered_ts(rng, ne, span_s, t0=T0):
    return t0 + np.sort(rng.integers(0, span_s * US, ne))


def _files(rng, ne, nf, bad=0.03):
    """Random files with the last one present and events outside the manifest
    (-1 and >= nf)."""
    f = rng.integers(0, nf, ne)
    if ne > 2:
        f[rng.integers(0, ne)] = nf - 1
        b = np.flatnonzero(rng.random(ne) < bad)
        f[b[::2]] = -1
        f[b[1::2]] = nf + rng.integers(0, 5, b[1::2].size)
    return f


def k32_log(seed, ne, nf, span_s=600):
    """Time-ordered, files unordered: the 32-bit route with a sort."""
    rng = np.random.default_rng(seed)
    f = _files(rng, ne, nf)
    if ne == 2:
        f[:] = [nf - 1, 0]
    return _fill(rng, f, _ordered_ts(rng, ne, span_s), nf)


def k64_log(seed, ne, nf, span_s=600, t0=T0, null_frac=0.02):
    """Not time-ordered, some null timestamps: the general route with a sort."""
    rng = np.random.default_rng(seed)
    f = _files(rng, ne, nf)
    ts = t0 + rng.integers(0, span_s * US, ne)
    if span_s > 1 and ne > 1:  # the exact second range span_s - 1
        ts[0], ts[1] = t0 + (span_s - 1) * US + 5, t0
    ts[rng.random(ne) < null_frac] = NULL
    if ne == 2:
        f[:] = [nf - 1, 0]
        ts[:] = [t0 + 1, t0]
    elif ne > 2:
        ts[2] = NULL
    return _fill(rng, f, ts, nf)


def same_digit_k64():
    """Every event of one file (66000 of 70000), seconds unordered: the two
    upper radix passes see one digit only."""
    rng = np.random.default_rng(71)
    ne, nf = 9000, 70_000
    return _fill(rng, np.full(ne, 66_000), T0 + rng.integers(0, 600 * US, ne), nf)


def same_digit_k32():
    """Time-ordered, every file id = 5 mod 256: the first radix pass sees one
    digit only (the third two)."""
    rng = np.random.default_rng(72)
    ne, nf = 9000, 70_000
    f = 256 * rng.integers(0, nf // 256, ne) + 5
    return _fill(rng, f, _ordered_ts(rng, ne, 600), nf)


def invalid_only(ordered: bool):
    rng = np.random.default_rng(73)
    ne, nf = 5000, 300
    f = np.where(rng.random(ne) < 0.5, -1, nf + rng.integers(0, 9, ne))
    ts = _ordered_ts(rng, ne, 600) if ordered else T0 + rng.integers(0, 600 * US, ne)
    return _fill(rng, f, ts, nf)


STABLE_NF = 300
STABLE_HOT = {3: 5 * 64, 130: 3 * RS_CHUNK, 257: RS_TILE}  # hot file -> the boundary it straddles


def stability_log():
    """Time-ordered log on the 32-bit route.  Around each boundary B (a lane-64,
    a chunk-256 and the tile-4096 boundary of rs_scatter) one hot file has ten
    events at every other position B - 10 .. B + 8 with seconds s, s, s, s+1,
    s+1 | s+1, s+1, s+2, s+2, s+2: second s + 1 straddles B and is the file's
    only second with four events, so a sort that moves the events after B
    before the ones in front of it (or reverses either side) splits the run
    and per_file_run reports 3."""
    rng = np.random.default_rng(74)
    ne = RS_TILE + 700
    others = np.setdiff1d(np.arange(STABLE_NF), list(STABLE_HOT))
    f = rng.choice(others, ne)
    sec = np.zeros(ne, dtype=np.int64)
    for B in sorted(STABLE_HOT.values()):
        sec[B - 5:] += 1
        sec[B + 4:] += 1
    for h, B in STABLE_HOT.items():
        f[B - 10:B + 10:2] = h
    ts = T0 + sec * US + np.arange(ne)  # non-decreasing, ne < 1e6 us
    return _fill(rng, f, ts, STABLE_NF)


def unstable_order(f, nf, hot, B):
    """The stable order by file, except that the hot file's events from
    position B on come before its earlier ones."""
    key = np.where((f >= 0) & (f < nf), f, nf).astype(np.int64)
    order = np.argsort(key, kind="stable")
    mine = order[key[order] == hot]
    order[key[order] == hot] = np.concatenate([mine[mine >= B], mine[mine < B]])
    return order


PF_NF = 4 * 64 + 37


def per_file32_log():
    """Time-ordered; the 64-file groups of per_file32 hold 768 events (staged),
    769 (global memory), none, the events of one file only, and the last
    group has 37 files; invalid events are mixed in."""
    rng = np.random.default_rng(75)
    parts = [rng.integers(0, 64, PER_FILE_STAGE),
             64 + rng.integers(0, 64, PER_FILE_STAGE + 1),
             np.full(400, 3 * 64 + 17),
             4 * 64 + rng.integers(0, 37, 500),
             np.full(40, -1), PF_NF + rng.integers(0, 3, 40)]
    f = rng.permutation(np.concatenate(parts))
    return _fill(rng, f, _ordered_ts(rng, f.size, 20), PF_NF)


def group_spans(f, nf):
    """Events per 64-file group: per_file32's span of sorted values."""
    v = f[(f >= 0) & (f < nf)]
    return np.bincount(v // 64, minlength=-(-nf // 64))


def sorted_k32():
    """Time-ordered and grouped by file: the 32-bit route skips the sort."""
    rng = np.random.default_rng(76)
    ne, nf = 6000, 700
    f = np.sort(rng.integers(0, nf, ne))
    f[-30:] = nf + 2  # invalid keys sort last
    return _fill(rng, f, _ordered_ts(rng, ne, 60), nf)


def sorted_k64():
    """File-major, second-ordered, nulls last per file: the general route
    skips the sort."""
    rng = np.random.default_rng(77)
    ne, nf = 6000, 700
    f = rng.integers(0, nf, ne)
    ts = T0 + rng.integers(0, 60 * US, ne)
    ts[rng.random(ne) < 0.05] = NULL
    o = np.lexsort((np.where(ts == NULL, np.iinfo(np.int64).max, ts), f))
    return _fill(rng, f[o], ts[o], nf)


def sorted_pair():
    rng = np.random.default_rng(78)
    return _fill(rng, np.array([0, 1]), np.array([T0, T0 + 5]), 2)


def single_event():
    rng = np.random.default_rng(79)
    return _fill(rng, np.array([1]), np.array([T0 + 7]), 3)


def nulls_sbits32():
    """General route at sbits = 32, from before the epoch: file 0 has only
    null timestamps (the null code 2^32 - 1 is per_file's initial `prev`),
    file 1 real seconds and nulls, file 2 the seconds -1 and -2 (floor of a
    negative), file 5 no event."""
    rng = np.random.default_rng(80)
    lo = -(1 << 30) * US
    f = np.array([0] * 7 + [1] * 9 + [2] * 6 + [3, 4, 3, -1])
    ts = np.array([NULL] * 7
                  + [5 * US, NULL, 5 * US + 1, NULL, 6 * US, NULL, 5 * US + 9, NULL, NULL]
                  + [-1, -US, -US - 1, -2 * US, -1 - US, -999_999]
                  + [lo - 1, lo + ((1 << 31) + 3) * US, lo, 77])
    o = rng.permutation(f.size)
    return _fill(rng, f[o], ts[o], 6)


# natural entries: groupby_resident declines without a switch
WIDE_CLIENT = (1 << 31) - 2


def natural_general(span_s=1 << 31):
    """nf = 4, not time-ordered, nulls, second range exactly span_s, one
    client 2^31 - 2: the payload needs 2 + 31 + 32 + 0 = 65 bits."""
    rng = np.random.default_rng(81)
    f = np.array([2, 0, 3, 0, 2, -1, 0, 1, 2, 2, 4, 0])
    ts = np.array([T0 + 5, NULL, T0 + span_s * US + 999_999, T0 + 2 * US, T0 + 6, T0 + 9, NULL,
                   T0, T0 + US, T0 + 999_999, T0 + 3, T0 + 2 * US + 1])
    fl, op, cl, ts, prim = _fill(rng, f, ts, 4)
    cl, prim = cl.copy(), prim.copy()
    cl[0], prim[2] = WIDE_CLIENT, WIDE_CLIENT  # local through the wide id
    return _ro(fl, op, cl, ts, prim)


def natural_k32():
    """nf = 1100, time-ordered, no nulls, second range exactly 2^29 - 1, the
    same wide client: 2 + 31 + 30 + 2 = 65 bits; make_keys32's second field
    reaches its top value."""
    rng = np.random.default_rng(82)
    ne, nf = 5000, 1100
    ts = _ordered_ts(rng, ne, (1 << 29) - 1)
    ts[0], ts[-3:] = T0, T0 + ((1 << 29) - 1) * US + np.array([0, 0, 999_999])
    fl, op, cl, ts, prim = _fill(rng, _files(rng, ne, nf), ts, nf)
    cl, fl, prim = cl.copy(), fl.copy(), prim.copy()
    fl[-3:] = 1099
    cl[-1], prim[1099] = WIDE_CLIENT, WIDE_CLIENT
    return _ro(fl, op, cl, ts, prim)


def empty_manifest(ordered: bool):
    rng = np.random.default_rng(83)
    ne = 1000
    f = rng.integers(-1, 50, ne)
    if ordered:
        ts = _ordered_ts(rng, ne, 600)
    else:
        ts = T0 + rng.integers(0, 600 * US, ne)
        ts[rng.random(ne) < 0.05] = NULL
        ts[int(np.argmax(ts))] = NULL  # the largest is not simply the last or the plain max
    return _fill(rng, f, ts, 0)


R32_NF = (255, 256, 65_535, 65_536)                       # 1, 2, 2, 3 passes
# general route, (n_files, seconds): end_bit = sbits + fbits + 1
R64 = ((1, 1), (100, 100), (1000, 600), (1000, 100_000), (1 << 20, (1 << 31) + 1))
R64_PASSES = (1, 2, 3, 4, 7)
TILE_N = (2, 255, 256, 257, 4095, 4096, 4097)
SCAN_N = 257 * RS_TILE + 1

SORT_CASES = {}
for _nf in R32_NF:
    SORT_CASES["r32-nf%d" % _nf] = functools.partial(k32_log, 100 + _nf % 97, 20_000, _nf)
for (_nf, _s), _p in zip(R64, R64_PASSES):
    SORT_CASES["r64-p%d" % _p] = functools.partial(
        k64_log, 200 + _p, 30_000, _nf, _s, T0 if _p < 7 else -(1 << 30) * US, 0.3 if _p == 1 else 0.02)
for _n in TILE_N:
    SORT_CASES["n32-%d" % _n] = functools.partial(k32_log, 300 + _n % 89, _n, 300)
    SORT_CASES["n64-%d" % _n] = functools.partial(k64_log, 400 + _n % 89, _n, 300)
SORT_CASES.update({
    "scan32": functools.partial(k32_log, 501, SCAN_N, 3000),
    "scan64": functools.partial(k64_log, 502, SCAN_N, 3000),
    "digit64": same_digit_k64, "digit32": same_digit_k32,
    "invalid32": functools.partial(invalid_only, True),
    "invalid64": functools.partial(invalid_only, False),
    "stable": stability_log, "perfile32": per_file32_log,
    "sorted32": sorted_k32, "sorted64": sorted_k64, "pair": sorted_pair, "one": single_event,
    "nulls32bit": nulls_sbits32,
})
NATURAL_CASES = {"natural64": natural_general, "natural32": natural_k32,
                 "nomanifest-ordered": functools.partial(empty_manifest, True),
                 "nomanifest-shuffled": functools.partial(empty_manifest, False),
                 "refused": functools.partial(natural_general, 1 << 32)}


@functools.lru_cache(maxsize=4)
def sort_case(name):
    return (SORT_CASES.get(name) or NATURAL_CASES[name])()


@functools.lru_cache(maxsize=4)
def sort_expect(name):
    f, op, cl, ts, prim = sort_case(name)
    exp, mx = fo.counts_from_arrays(f, op, cl, ts, prim, prim.size)
    exp.setflags(write=False)
    return exp, NULL if mx is None else mx


# ---- client-id width ---------------------------------------------------------
WIDTH_CMAX = ((1 << 30) - 2, (1 << 30) - 1, 1 << 30, (1 << 31) - 2, (1 << 31) - 1)  # cbits 30..32
# kernel -> (events, files, seconds, switch)
WIDTH_SHAPES = {"gb_bucket_wave4": (200_000, 2000, 30, None),
                "gb_bucket_wave": (200_000, 2000, 30, "CDR_GB_BALLOT"),
                "gb_bucket_dense": (200_000, 20_000, 200, "CDR_GB_BLOCK"),
                "gb_bucket": (100_000, 3000, 86_400, None),
                "gb_bucket_big": (200_000, 50, 100_000, None)}
INT32_MAX = (1 << 31) - 1


@functools.lru_cache(maxsize=2)
def width_log(kernel, cmax):
    """A log of the kernel's shape whose largest client is cmax: half the
    clients spread over [0, cmax], primaries up to 2^31 - 1, and 4000 events
    sent by their file's primary (the primaries at or above 2^30 included,
    where cmax allows it); event 0 is a READ by client cmax, its file's
    primary."""
    ne, nf, span, _ = WIDTH_SHAPES[kernel]
    rng = np.random.default_rng(WIDTH_CMAX.index(cmax) * 10 + list(WIDTH_SHAPES).index(kernel))
    f = _files(rng, ne, nf)
    ts = T0 + rng.integers(0, span * US, ne)
    ts[0], ts[1] = T0, T0 + (span - 1) * US
    ts[rng.random(ne) < 0.01] = NULL
    op = rng.integers(0, 3, ne).astype(np.uint8)
    cl = np.where(rng.random(ne) < 0.5, rng.integers(0, cmax + 1, ne), rng.integers(-1, 4, ne))
    cl[rng.random(ne) < 0.02] = -3
    prim = np.where(rng.random(nf) < 0.6, rng.integers(0, cmax + 1, nf), rng.integers(-2, 4, nf))
    prim[rng.integers(0, nf, max(2, nf // 20))] = INT32_MAX
    prim[rng.integers(0, nf, max(2, nf // 20))] = cmax
    valid = np.flatnonzero((f >= 0) & (f < nf))
    hit = valid[(prim[f[valid]] >= 0) & (prim[f[valid]] <= cmax)]
    big = hit[prim[f[hit]] >= min(cmax, 1 << 30)]
    hit = np.concatenate([big[:2000], hit[:2000]])
    cl[hit] = prim[f[hit]]
    f[0], op[0], cl[0] = nf - 1, 2, cmax
    prim[nf - 1] = cmax
    return _ro(f.astype(np.int32), op, cl.astype(np.int32), ts.astype(np.int64),
               prim.astype(np.int32))


# ---- exchange ------------------------------------------------------------------
X_NF = 5000
X_HOLE = (100, 120)  # no event names these files
X_NE = (0, 1, 255, 256, 257, 70_001, FIN_THREADS + 513)
X_CLIENTS = (-1, -3, 0, X_CLIENT_LIM - 1)
XREC = np.dtype([("ts", "<i8"), ("file", "<i4"), ("cop", "<i4")])


@functools.lru_cache(maxsize=2)
def exchange_log(ne, nulls="some"):
    """Events with every listed client and op value, files -1 and >= X_NF,
    none in X_HOLE; about 1 % (or all) timestamps null."""
    rng = np.random.default_rng(600 + ne % 1009)
    f = rng.integers(-1, X_NF + 3, ne)
    f[(f >= X_HOLE[0]) & (f < X_HOLE[1])] += X_HOLE[1] - X_HOLE[0]
    op = (np.arange(ne) % 3).astype(np.uint8)
    cl = rng.choice(np.array(X_CLIENTS + (1, 2, 3, 77, -X_CLIENT_LIM)), ne)
    cl[:min(ne, 4)] = X_CLIENTS[:min(ne, 4)]
    if ne >= 8:
        f[4:7], cl[7] = [-1, X_NF, X_NF + 2], -X_CLIENT_LIM
    ts = T0 + rng.integers(-5 * US, 600 * US, ne)
    if nulls == "all":
        ts[:] = NULL
    elif ne:
        ts[rng.random(ne) < 0.01] = NULL
        ts[int(np.argmax(ts))] = NULL
    prim = rng.integers(-2, 4, X_NF)
    return _ro(f.astype(np.int32), op, cl.astype(np.int32), ts.astype(np.int64),
               prim.astype(np.int32))


def exchange_bounds(kind, nranks, nf=X_NF):
    """nranks + 1 non-decreasing bounds.  even: [0, nf] in equal parts; runs:
    the same with runs of empty owners; window: bounds[0] > 0 and
    bounds[nranks] < nf (with empty owners too when nranks > 2); hole: a
    window inside X_HOLE, which no event falls in."""
    if kind == "hole":
        return np.linspace(X_HOLE[0], X_HOLE[1], nranks + 1).astype(np.int64)
    lo, hi = (0, nf) if kind != "window" else (nf // 7, nf - nf // 5)
    b = np.linspace(lo, hi, nranks + 1).astype(np.int64)
    if kind != "even" and nranks > 2:
        b[1:-1] = np.sort(np.repeat(b[1:-1:3], 3)[:nranks - 1])
    return b


def exchange_expect(f, op, cl, ts, bounds):
    """counts per owner, each owner's records sorted, the non-null maximum."""
    nr = bounds.size - 1
    sent = np.flatnonzero((f >= bounds[0]) & (f < bounds[nr]))
    owner = np.searchsorted(bounds, f[sent], side="right") - 1
    counts = np.bincount(owner, minlength=nr).astype(np.int64)
    rec = np.zeros(sent.size, dtype=XREC)
    rec["ts"], rec["file"] = ts[sent], f[sent]
    rec["cop"] = ((cl[sent].astype(np.int64) << 8) | op[sent]).astype(np.uint32).view(np.int32) \
        if sent.size else 0
    o = np.lexsort((rec["cop"], rec["file"], rec["ts"], owner))
    real = ts[ts != NULL]
    return counts, rec[o], int(real.max()) if real.size else NULL


def sort_records(raw, counts):
    """The packed bytes as records, each owner's region sorted."""
    n = int(counts.sum())
    rec = np.frombuffer(raw[:16 * n].tobytes(), dtype=XREC)
    owner = np.repeat(np.arange(counts.size), counts)
    return rec[np.lexsort((rec["cop"], rec["file"], rec["ts"], owner))]


# ---- K6 ------------------------------------------------------------------------
FIN_CASES = ("one", "constant", "nowrites", "total0", "allnan", "future", "lastbit", "two53",
             "grid")


@functools.lru_cache(maxsize=2)
def fin_case(name):
    """(counts (n, 6), creation seconds, observation end) for K6."""
    rng = np.random.default_rng(700 + FIN_CASES.index(name))
    n = {"one": 1, "grid": FIN_THREADS + 3}.get(name, 1500)
    obs = 1.7e9 + 0.123456
    af = rng.integers(0, 1000, n)
    c = np.zeros((n, 6), dtype=np.int64)
    c[:, 0] = c[:, 4] = af
    c[:, 1] = rng.integers(0, af + 1)
    c[:, 2] = af - c[:, 1]
    c[:, 3] = rng.integers(0, af + 1)
    c[:, 5] = np.where(af > 0, np.maximum(rng.integers(0, af + 1), 1), 0)
    cr = np.where(rng.random(n) < 0.05, np.nan, 1.69e9 + rng.integers(0, 10 ** 6, n)).astype(float)
    if name == "constant":
        c[:] = [40, 10, 30, 20, 40, 7]
        cr[:] = 1.69e9 + 17
    elif name == "nowrites":
        c[:, 2] += c[:, 1]
        c[:, 1] = 0
    elif name == "total0":
        c[::3] = 0              # no accesses: locality 1.0
        c[1::3, 3] = 0          # locality 0
        c[1::3, 0] = c[1::3, 4] = np.maximum(c[1::3, 0], 1)
        c[2::3, 3] = c[2::3, 4] = c[2::3, 0] = np.maximum(c[2::3, 0], 1)  # locality 1
    elif name == "allnan":
        cr[:] = np.nan
    elif name == "future":
        cr[::2] = obs + rng.integers(1, 10 ** 6, cr[::2].size)
    elif name == "lastbit":
        obs = 12345.678  # creation times of 0, 1 and 2 ulp(obs): three adjacent ages
        cr[:] = 0.0
        cr[::2] = np.spacing(obs)
        cr[5] = 2 * np.spacing(obs)
    elif name == "two53":
        big = (1 << 53) + rng.integers(-3, 12, n)
        c[:, 0] = c[:, 4] = big
        c[:, 5] = big - rng.integers(0, 5, n)
        c[:, 3] = big - rng.integers(0, 9, n)
        c[:, 1] = rng.integers(0, 100, n)
        c[:, 2] = big - c[:, 1]
    return _ro(c, cr) + (obs,)

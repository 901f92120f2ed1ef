"""csrc/csv_digits.h on the host: the cell text of the device CSV writer equals
compute_features.java_double_legacy / str(int(v)) (CPU; needs g++)."""
import math
import os
import random
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import csv_cases as cc
from conftest import REPO

N5_BITS = [(5 ** i).bit_length() for i in range(27)]
ARM_CODE = {"special": 0, "integer": 1, "w32": 2, "w64": 3, "big": 4}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the host check of csv_digits.h cannot be built")
    exe = str(tmp_path_factory.mktemp("csvd") / "csv_digits_check")
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-std=c++17",
                    os.path.join(REPO, "tools", "csv_digits_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, vals, mode):
    out = subprocess.run([exe, mode], input=struct.pack(f"<{len(vals)}d", *vals),
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    return out.splitlines()


def host_arm(x, n_sig=53):
    """Which arm _legacy_digits takes for x (a restatement of its width tests):
    special, integer, w32, w64 or big."""
    if x != x or math.isinf(x) or x == 0.0:
        return "special"
    bits = cc.bits_of(x)
    fract = (bits & ((1 << 52) - 1)) | (1 << 52)
    bin_exp = ((bits >> 52) & 0x7FF) - 1023
    tail = (fract & -fract).bit_length() - 1
    n_fract = 53 - tail
    n_tiny = max(0, n_fract - bin_exp - 1)
    if n_tiny == 0 and -21 <= bin_exp <= 62:
        return "integer"
    mant = struct.unpack("<d", struct.pack("<Q", 0x3FF0000000000000 | (fract & ((1 << 52) - 1))))[0]
    dec = math.floor((mant - 1.5) * 0.289529654 + 0.176091259 + bin_exp * 0.301029995663981)
    b5, s5 = max(0, -dec), max(0, dec)
    b2, s2 = b5 + n_tiny + bin_exp, s5 + n_tiny
    m2 = b2 - n_sig
    b2 -= n_fract - 1
    common = min(b2, s2)
    b2, s2, m2 = b2 - common, s2 - common, m2 - common
    if n_fract == 1:
        m2 -= 1
    if m2 < 0:
        b2, s2 = b2 - m2, s2 - m2
    b_bits = n_fract + b2 + (N5_BITS[b5] if b5 < 27 else 3 * b5)
    ts_bits = s2 + 1 + (N5_BITS[s5 + 1] if s5 + 1 < 27 else 3 * (s5 + 1))
    if b_bits < 32 and ts_bits < 32:
        return "w32"
    return "w64" if b_bits < 64 and ts_bits < 64 else "big"


def carried_through_nine(x):
    """The host's digits were rounded up out of a truncation that ends in 9."""
    from compute_features import _legacy_digits

    bits = cc.bits_of(x)
    fract = (bits & ((1 << 52) - 1)) | (1 << 52)
    digits, exp = _legacy_digits(((bits >> 52) & 0x7FF) - 1023, fract, 53)
    n = len(digits)
    trunc = math.floor(Fraction(abs(x)) * Fraction(10) ** (n - exp))  # exact, n digits
    return int("".join(map(str, digits))) == trunc + 1 and trunc % 10 == 9


def check_float_digits(exe):
    """Digits and exponent of 4000 non-integer float32 values with 24 significant
    bits; returns how many took the 32-bit arm."""
    from compute_features import _legacy_digits

    rng = random.Random(5)
    vals = []
    while len(vals) < 4000:
        v = float(np.float32(rng.uniform(-1, 1) * 10 ** rng.randint(-6, 6)))
        if v != int(v) and 2.0 ** -100 < abs(v):
            vals.append(v)
    lines = run(exe, vals, "float")
    w32 = 0
    for v, line in zip(vals, lines):
        bits = cc.bits_of(v)
        fract = (bits & ((1 << 52) - 1)) | (1 << 52)
        digits, exp = _legacy_digits(((bits >> 52) & 0x7FF) - 1023, fract, 24)
        a = host_arm(v, 24)
        assert line == f"{''.join(map(str, digits))} {exp}\t{ARM_CODE[a]}", (v, line, digits, exp, a)
        w32 += a == "w32"
    return w32


def test_double_text_equals_java_double_legacy(checker):
    vals, exp = cc.double_cases()
    lines = run(checker, vals, "double")
    assert lines[-1].startswith("#bits ") and len(lines) == len(vals) + 1
    # the limbs of the multi-word arm (5 x 32 bits, csv_digits.h) never overflow
    assert int(lines[-1].split()[1]) <= 160, lines[-1]
    arm_name = {"0": "special", "1": "integer", "2": "w32", "3": "w64", "4": "big"}
    arms = dict.fromkeys(["special", "integer", "w32", "w64", "big"], 0)
    layouts = {"plain": 0, "small": 0, "sci": 0}
    carried = 0
    deferred = set()
    for v, e, line in zip(vals, exp, lines):
        txt, arm = line.split("\t")
        if txt == "DEFER":
            deferred.add(v)
            assert e is None, (v, e)
            continue
        assert txt == e, (v, txt, e)
        assert len(txt) <= 26
        a = host_arm(v)
        assert arm_name[arm] == a, (v, arm, a)
        arms[a] += 1
        if a == "special":
            continue
        body = txt.lstrip("-")
        layouts["sci" if "E" in body else ("small" if body.startswith("0.") else "plain")] += 1
        if a != "integer" and carried < 20:
            carried += carried_through_nine(v)
    assert deferred == set(cc.OUTSIDE) | {5e-324, -5e-324, 1.7976931348623157e308,
                                          -1.7976931348623157e308}
    # The 32-bit arm: after the m2 < 0 rescue b2 >= n_sig + 1 - n_fract, so b_bits >=
    # n_sig + 2, which is 55 for a double: no double reaches it (Java takes it for
    # floats, n_sig = 24).  Its inputs are therefore float32 values pushed through
    # the digit routine with n_sig = 24, against _legacy_digits with n_sig = 24.
    assert arms["w32"] == 0
    arms["w32"] = check_float_digits(checker)
    assert arms["special"] >= 5 and all(arms[a] >= 500 for a in ("integer", "w32", "w64", "big")), arms
    assert carried >= 20
    assert all(c >= 20 for c in layouts.values()), layouts


def test_long_text_equals_str_int(checker):
    vals = cc.LONGS + [-v for v in cc.LONGS] + cc.LONGS_DEFERRED
    lines = run(checker, vals, "long")
    assert len(lines) == len(vals)
    for v, txt in zip(vals, lines):
        if v in cc.LONGS_DEFERRED or v != v:
            assert txt == "DEFER", (v, txt)
        else:
            assert txt == str(int(v)), (v, txt)

"""Arithmetic behind the one-read bound extract (csrc/oz2_scale.hip, stage_panel_body), on the CPU.

A bound byte is a = ceil(|x| 2^s0) with s0 = 5 - ilogb(row maximum).  The one-read form writes tile t of a row with the provisional shift
s_t = 5 - ilogb(maximum over tiles 0 .. t) = s0 + d, d >= 0, and corrects the byte afterwards from the byte alone:
    ceil(ceil(y 2^d) / 2^d) = ceil(y),   i.e.   a = (a'' + 2^d - 1) >> d   (d >= 8: a'' > 0 ? 1 : 0, as a'' <= 64).
The identity is exact in real numbers; ldexp is not where its result falls below the normal range, so the kernel recomputes rows with
s0 + (a lower bound of the smallest exponent of a nonzero element) < -1022, or with an infinite maximum, in the two-pass order."""
from fractions import Fraction
import math

import numpy as np

TK = 128


def rescale(a2, d):
    """What the kernel applies to a provisional byte (four at a time, as a word)."""
    return (1 if a2 > 0 else 0) if d >= 8 else (a2 + (1 << d) - 1) >> d


def test_identity_on_rationals():
    """Every provisional byte a'' in 0 .. 64 and every d in 0 .. 70: all real y >= 0 with ceil(y 2^d) = a'' have ceil(y) = rescale(a'', d).  Checked at
    both ends of the interval ((a'' - 1) / 2^d, a'' / 2^d] of such y (ceil is monotone: the ends decide), in exact rational arithmetic."""
    for d in range(71):
        for a2 in range(65):
            ys = [Fraction(a2, 1 << d)]
            if a2 > 0:
                ys.append(Fraction(a2 - 1, 1 << d) + Fraction(1, 1 << (d + 90)))
            for y in ys:
                assert math.ceil(y * (1 << d)) == a2
                assert math.ceil(y) == rescale(a2, d), (a2, d, y)
            # the word form of the kernel: four bytes at once, no carry between them
            w = a2 * 0x01010101
            if d >= 8:
                got = ((w + 0x7F7F7F7F) >> 7) & 0x01010101
            else:
                got = ((w + ((1 << d) - 1) * 0x01010101) >> d) & ((0xFF >> d) * 0x01010101)
            assert got == rescale(a2, d) * 0x01010101, (a2, d)


def ilogb0(x):
    return 0 if x == 0 else (2 ** 31 - 1 if math.isinf(x) else math.frexp(x)[1] - 1)


def byte(x, s):
    """(int)ceil(ldexp(|x|, s)) as the device computes it: IEEE ldexp (rounds to nearest where the result is subnormal)."""
    v = np.ldexp(np.abs(x), s)
    return np.where(np.isfinite(v), np.ceil(np.where(np.isfinite(v), v, 0)), 0).astype(np.int64)


def two_pass(row):
    fin = row[~np.isnan(row)]
    am = float(np.max(np.abs(fin))) if fin.size else 0.0
    s0 = 5 - ilogb0(am)
    return s0, byte(row, max(s0, -5000))


def one_read(row):
    """The kernel's order on one row: provisional bytes per tile, rescale by d = s_t - s0, hazard flag."""
    k = row.size
    ex, none = None, True
    prov, st = np.zeros(k, np.int64), []
    emin = None
    for t0 in range(0, k, TK):
        x = row[t0:t0 + TK]
        ax = np.abs(x[~np.isnan(x)])
        nz = ax[(ax != 0) & np.isfinite(ax)]
        if ax.size and ax.max() > 0:
            e = ilogb0(float(ax.max()))
            ex = e if none else max(ex, e)
            none = False
        if nz.size:  # the kernel's lower bound: a subnormal counts as 2^-1074
            lo = float(nz.min())
            e = -1074 if lo < 2.0 ** -1022 else ilogb0(lo)
            emin = e if emin is None else min(emin, e)
        s_t = 5 if none else 5 - min(ex, 4096)
        st.append(s_t)
        prov[t0:t0 + TK] = byte(x, s_t)
    s0 = 5 if none else 5 - ex
    hazard = (not none) and (ex == 2 ** 31 - 1 or (emin is not None and s0 + emin < -1022))
    out = prov.copy()
    for i, s_t in enumerate(st):
        d = 0 if none else s_t - max(s0, 5 - 4096)
        assert d >= 0
        out[i * TK:(i + 1) * TK] = [rescale(int(a), min(d, 64)) for a in prov[i * TK:(i + 1) * TK]]
    return s0, out, hazard


def test_rescale_equals_two_pass_except_on_flagged_rows():
    """Random doubles over the whole exponent range in rows with planted maxima: the provisional-plus-rescale bytes equal the two-pass bytes on every
    row the hazard rule does not flag; flagged rows exist in the sample (the rule is exercised) and so do rows where the bytes would differ."""
    rng = np.random.default_rng(2024)
    nrows, k = 400, 5 * TK
    flagged = differing = clean = 0
    for r in range(nrows):
        kind = r % 5
        if kind == 0:    # full exponent range in one row
            e = rng.integers(-1074, 1023, k)
        elif kind == 1:  # a narrow band somewhere in the range
            e = rng.integers(-1070, 1000) + rng.integers(0, 24, k)
        elif kind == 2:  # subnormal and near-subnormal rows
            e = rng.integers(-1074, -1000, k)
        elif kind == 3:  # maxima rising tile by tile
            e = rng.integers(-300, 300) + np.repeat(np.cumsum(rng.choice([1, 6, 7, 8, 40], k // TK)), TK) + rng.integers(-3, 1, k)
        else:            # a wide band: more than 1022 + 52 binades below the maximum is where ldexp underflows
            e = rng.integers(-60, 1023) - rng.integers(0, 1100, k)
        e = np.clip(e, -1074, 1023)
        row = np.ldexp(rng.uniform(1.0, 2.0, k), e) * rng.choice([-1.0, 1.0], k)
        row[rng.integers(0, k, 3)] = 0.0
        if r % 7 == 0:  # a planted maximum in a late tile
            row[rng.integers(k - TK, k)] = np.ldexp(1.5, min(1023, int(e.max()) + int(rng.integers(1, 50))))
        s0, want = two_pass(row)
        s1, got, hazard = one_read(row)
        assert s0 == s1
        same = np.array_equal(want, got)
        flagged += hazard
        differing += not same
        clean += (not hazard) and same
        assert same or hazard, f"row {r} (kind {kind}): bytes differ on a row the hazard rule does not flag"
    assert flagged > 0 and differing > 0 and clean > nrows // 3, (flagged, differing, clean)


def test_non_finite_rows_are_flagged():
    rng = np.random.default_rng(5)
    row = rng.uniform(-1, 1, 3 * TK)
    row[200] = np.inf
    row[5] = np.nan
    assert one_read(row)[2]
    row[200] = 0.5
    s0, want = two_pass(row)
    s1, got, hazard = one_read(row)  # NaN alone never wins the maximum: an ordinary row, its NaN byte is 0 both ways
    assert not hazard and s0 == s1 and np.array_equal(want, got)

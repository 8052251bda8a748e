"""Number parsing (ops/text.py parse_f64 / parse_i64; tx::parse_f64 of
csrc/hip/text_parse.h in text_parse_f64_kernel and in the fused CSV fold;
text_parse_i64_kernel) against an oracle that shares nothing with the project:
one regular expression for the grammar, Python's correctly rounded float() and
int() for the value.

Distance between two doubles = the absolute difference of their bit patterns
read as integers, signs required equal: ulps among the normal doubles, steps
of 2^-1074 among the subnormals, 1 from DBL_MAX to inf.

Classes and what each must give on the GPU:
  exact       value m * 10^k, m < 2^53 without its trailing zeros, |k| <= 22,
              written every way that reaches it: distance 0.
  round-trip  repr / %.17g / %.17e of random doubles of every exponent,
              DBL_MIN, DBL_MAX, 5e-324 and their neighbours: distance <= B.
  long        20..40 significant digits (the parser keeps 19), exponent
              -330..310, with tokens whose late digits decide the rounding:
              distance <= B.
  range ends  around DBL_MAX + half an ulp and around 2^-1075: distance <= B;
              exponents of twenty digits and zeros: distance 0.
  malformed   NaN (f64) / 0 (i64), the error word, ValueError with check.

B = 3.  Outside the exact class the parser keeps 19 digits (under 2^-59
relative), converts them to a double (0.5 ulp), multiplies by a correctly
rounded 5^k from a table (0.5 ulp in the constant, 0.5 ulp in the product) and
scales by 2^k with ldexp (exact, or one rounding into a subnormal): under 1.6
ulp, so at most 2 steps from the correctly rounded double; B leaves one spare.

Measured on an MI355X, worst distance per class against float() (the tests
print them; conversion, multiply and ldexp are IEEE operations, so a CPU
emulation of the same steps gives the same figures bit for bit):
  exact 0 (4392 tokens) | round-trip 2 (4998 tokens, 73.1 % at 0) |
  long 2 (3809, 62.1 % at 0) | range ends 1 (1018, 53.0 % at 0) |
  CSV fields 2 (2665, 82.2 % at 0).
"""
import math
import os
import random
import re
import sys
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import csv_modules as CM  # noqa: E402

from lua_mapreduce_1_amd.ops import text as TX  # noqa: E402

B = 3

WS = b" \t\n\v\f\r"
_W = rb"[ \t\n\v\f\r]*"
F64_RE = re.compile(_W + rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?" + _W)
I64_RE = re.compile(_W + rb"[+-]?[0-9]{1,19}" + _W)
DBL_MAX = sys.float_info.max
DBL_MIN = sys.float_info.min
TINY = 5e-324
T_INF = (2**54 - 1) * 2**970  # DBL_MAX + half an ulp: from here on float() gives inf
MAGN = np.int64(0x7FFFFFFFFFFFFFFF)


# -- the oracle ----------------------------------------------------------------
def oracle_f64(tok: bytes):
    """float() of a well-formed token, None for a malformed one."""
    if F64_RE.fullmatch(tok) is None:
        return None
    return float(tok.strip(WS).decode("ascii"))


def oracle_i64(tok: bytes):
    if I64_RE.fullmatch(tok) is None:
        return None
    v = int(tok.strip(WS).decode("ascii"))
    return v if -2**63 <= v < 2**63 else None


def parts(tok: bytes):
    """(negative, m, k) of a well-formed token: its value is m * 10^k exactly,
    m without trailing zeros (0: k = 0).  Integer arithmetic on the text."""
    assert F64_RE.fullmatch(tok) is not None, tok
    s = tok.strip(WS).decode("ascii").lower()
    neg = s.startswith("-")
    s = s.lstrip("+-")
    mant, _, e = s.partition("e")
    ip, _, fp = mant.partition(".")
    m, k = int(ip + fp), (int(e) if e else 0) - len(fp)
    if m == 0:
        return neg, 0, 0
    while m % 10 == 0:
        m, k = m // 10, k + 1
    return neg, m, k


def value(tok: bytes) -> Fraction:
    neg, m, k = parts(tok)
    assert abs(k) < 5000, tok  # (not for the twenty-digit exponents)
    v = Fraction(m) * Fraction(10) ** k
    return -v if neg else v


def bits(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).view(np.int64)


def distances(got, exp) -> np.ndarray:
    """Per element: |bit pattern difference| of the magnitudes; 2^62 where the
    signs differ or exactly one is a NaN, 0 where both are NaNs."""
    g, e = bits(got), bits(exp)
    d = np.abs((g & MAGN) - (e & MAGN))
    gn, en = np.isnan(np.asarray(got)), np.isnan(np.asarray(exp))
    d = np.where((g < 0) != (e < 0), np.int64(1) << 62, d)
    d = np.where(gn ^ en, np.int64(1) << 62, d)
    return np.where(gn & en, 0, d)


def test_distance_is_ulps_and_subnormal_steps():
    nxt = math.nextafter
    a = [1.0, DBL_MAX, 0.0, TINY, DBL_MIN, -1.0, 0.0, float("nan"), 1.0]
    b = [nxt(1.0, 2), math.inf, TINY, 3 * TINY, nxt(DBL_MIN, 0), -nxt(1.0, 0), -0.0, float("nan"), float("nan")]
    assert distances(a, b).tolist() == [1, 1, 1, 2, 1, 1, 1 << 62, 0, 1 << 62]


# -- span layout -----------------------------------------------------------------
def layout(tokens, sep=b";"):
    """Tokens joined by a byte no number contains: (text, starts, lens)."""
    starts, lens, pos = [], [], 0
    for t in tokens:
        starts.append(pos)
        lens.append(len(t))
        pos += len(t) + 1
    data = sep.join(tokens) + sep
    return (torch.frombuffer(bytearray(data), dtype=torch.uint8), torch.tensor(starts, dtype=torch.int64),
            torch.tensor(lens, dtype=torch.int32))


# -- corpora ---------------------------------------------------------------------
def _spellings(rng, m: int, k: int):
    """Ways to write m * 10^k (m > 0)."""
    d = str(m)
    n = len(d)
    out = ["%se%d" % (d, k), "%sE%+d" % (d, k), "%s.e%d" % (d, k), ".%se%d" % (d, k + n), "+.%se%d" % (d, k + n),
           "0.%se%d" % (d, k + n), "000%se%d" % (d, k), "000.000%se%d" % (d, k + n + 3),
           "%s.%se%d" % (d[0], d[1:], k + n - 1)]
    i = rng.randrange(0, n + 1)  # digits after the dot that an e+N cancels
    out.append("%s.%se%+d" % (d[:i] or "0", d[i:], k + n - i))
    z = rng.randrange(1, 30)  # trailing zeros, also past the 19 digits the parser keeps
    out += ["%s%se%d" % (d, "0" * z, k - z), "%s.%se%d" % (d, "0" * z, k), "%s%s.%se%d" % (d, "0" * z, "0" * z, k - z)]
    z = rng.randrange(1, 40)
    out.append("0.%s%se%d" % ("0" * z, d, k + n + z))
    if k >= 0:  # no exponent at all
        out.append(d + "0" * k)
        out.append(d + "0" * k + ".")
        out.append(d + "0" * k + ".000")
    elif -k < n:
        out.append(d[:n + k] + "." + d[n + k:])
    else:
        out.append("0." + "0" * (-k - n) + d)
        out.append("." + "0" * (-k - n) + d)
    return out


EXACT_FIXED = [b".5", b"5.", b"+.5", b"-.5", b"000.000123", b"0.000123", b"00012", b"+7", b"1" + b"0" * 25 + b"e-10",
               b"0." + b"0" * 400 + b"1e401", b"1" + b"0" * 400 + b"e-400", b"1e22", b"1e-22", b"-1E+22",
               b"9007199254740991", b"9007199254740991e22", b"9007199254740991e-22", b"90071992547409910e21",
               b"0.9007199254740991e38", b"999999999999999e22", b"999999999999999e-22", b"1e0", b"0", b"0.0",
               b"000", b"0e5", b".0", b"0.", b"0e-5", b"+0"] + [t.encode() for t in CM.GOOD]
# one step outside the exact class: exponent 23, mantissa 2^53 + 1
NEXT_TO_EXACT = [b"1e23", b"1e-23", b"-1e23", b"9007199254740993", b"9007199254740993e22", b"9007199254740993e-22",
                 b"9007199254740991e23", b"9007199254740991e-23", b"3e23", b"7e-23", b"123456789e23",
                 b"9007199254740992e23", b"9007199254740995", b"18014398509481985"]


@lru_cache(maxsize=None)
def exact_corpus():
    rng = random.Random(101)
    toks = list(EXACT_FIXED)
    for i in range(260):
        if i % 2:
            m = rng.randrange(1, 10 ** rng.randrange(1, 16))  # at most 15 digits
        else:
            m = rng.randrange(1, 2 ** rng.randrange(1, 54))   # below 2^53
        if i < 8:
            m = 2**53 - 1 - 2 * i
        m = m + 1 if m % 10 == 0 else m
        k = rng.choice([-22, 22, -21, 21]) if i % 5 == 0 else rng.randrange(-22, 23)
        for s in _spellings(rng, m, k):
            s = s if s[0] == "+" else rng.choice(["", "", "-", "+"]) + s
            toks.append(s.encode())
    base = [b"1.5", b"-2.5e-3", b"123456789012345", b".25"]
    for w in WS:  # each whitespace byte, on either side and both
        w = bytes([w])
        for t in base:
            toks += [w + t, t + w, w + w + t + w, w + t + w + w + w]
    toks.append(WS + b"7.5" + WS)
    return tuple(toks)


def _random_doubles(rng, n):
    out = []
    for _ in range(n):
        e = rng.randrange(0, 2047)  # every biased exponent, the subnormals' 0 included
        v = (e << 52) | rng.getrandbits(52)
        x = float(np.array([v], dtype=np.uint64).view(np.float64)[0])
        if x != 0.0:
            out.append(-x if rng.random() < 0.3 else x)
    return out


def _neighbours(x):
    return [y for y in (math.nextafter(x, 0.0), x, math.nextafter(x, math.inf)) if 0.0 < y < math.inf]


@lru_cache(maxsize=None)
def roundtrip_corpus():
    """(tokens, the doubles they were printed from)."""
    rng = random.Random(202)
    xs = _random_doubles(rng, 1400)
    xs += [rng.getrandbits(rng.randrange(1, 53)) * TINY or TINY for _ in range(100)]        # subnormals
    xs += [math.ldexp(1.0 + rng.random(), rng.randrange(-1022, -962)) for _ in range(100)]  # normal, below 1e-289
    for x in (DBL_MIN, DBL_MAX, TINY, 2.2250738585072014e-308, 1e-290, 1e-300, 1e-308, 1e-310, 1e-323, 1e300, 1e308,
              2.0**-1022, 2.0**-1023, 2.0**1023, 1e22, 1e23, 2.0**53, 2.0**63, 2.0**64, 0.1, 1 / 3):
        xs += _neighbours(x)
    toks, src = [], []
    for x in xs:
        for s in (repr(x), "%.17g" % x, "%.17e" % x):
            toks.append(s.encode())
            src.append(x)
    toks.append(b"2.2250738585072014e-308")
    src.append(DBL_MIN)
    for t in NEXT_TO_EXACT:
        toks.append(t)
        src.append(float(t))
    return tuple(toks), tuple(src)


def _sci(digits: str, x: int, rng) -> str:
    """digits[0].digits[1:] * 10^x, the dot put anywhere."""
    n = len(digits)
    i = rng.choice([0, 1, 1, n, rng.randrange(0, n + 1)])
    return "%s.%se%d" % (digits[:i], digits[i:], x - i + 1) if i < n else "%se%d" % (digits, x - n + 1)


@lru_cache(maxsize=None)
def long_corpus():
    """(random long tokens, tokens whose digits past the 19th decide the rounding)."""
    rng = random.Random(303)
    toks = []
    for _ in range(3000):
        n = rng.randrange(20, 41)
        d = str(rng.randrange(1, 10))
        d += "".join(rng.choice("0123456789") for _ in range(n - 2))
        d += str(rng.randrange(1, 10))
        toks.append((rng.choice(["", "-"]) + _sci(d, rng.randrange(-330, 311), rng)).encode())
    # 2^53 + 1 lies half way between two doubles: a late 1 sends it up, the 19 digits kept tie to even
    late = [b"9007199254740993." + b"0" * k + b"1" for k in (3, 4, 10, 23)]
    late += [b"900719925474.0993" + b"0" * k + b"1e4" for k in (3, 10)]
    late += [b"9007199254740992." + b"9" * k for k in (4, 10, 24)]
    for _ in range(400):
        # an integer half way between two doubles (17..19 digits), a hair above and a hair below
        e = rng.randrange(54, 63)
        x = (rng.getrandbits(52) | (1 << 52)) << (e - 52)
        mid = x + (1 << (e - 53))
        z = "0" * rng.randrange(19 - len(str(mid)), 12)
        late.append(("%d.%s1" % (mid, z)).encode())
        late.append(("%d.%s" % (mid - 1, "9" * (len(z) + 3))).encode())
    return tuple(toks), tuple(late)


@lru_cache(maxsize=None)
def range_corpus():
    """(tokens within B of float(), tokens whose result is beyond doubt: distance 0)."""
    rng = random.Random(404)
    near = []
    for _ in range(220):
        r = rng.getrandbits(rng.randrange(1, 968))
        near += [str(T_INF + r), str(T_INF - 1 - r)]          # 309 digits: inf / DBL_MAX
        near += ["%de%d" % ((T_INF + r) // 10**280 + 1, 280), "%de%d" % ((T_INF - 1 - r) // 10**280, 280)]  # 29 digits
    near += [str(T_INF), str(T_INF - 1), str(2**1024), str(2**1024 - 1), str(int(DBL_MAX)), "1.7976931348623157e308",
             "1.7976931348623158e308", "1.7976931348623159e308", "1.797693134862315807e308",
             "1.797693134862315808e308", "17976931348623157e292", "0.000017976931348623158e313", "1.8e308", "2e308",
             "1e309", "-1.7976931348623159e308", "-1.7976931348623158e308", "179769313486231580793e288",
             "179769313486231580794e288"]
    half = Fraction(1, 2**1075)  # half the smallest subnormal: at or below it float() gives 0
    for num, den in ((1, 1), (3, 2), (2, 1), (3, 1), (5, 1), (7, 2)):  # 1, 1.5, 2, 3, 5, 3.5 times 2^-1075
        v = half * num / den
        for nd in (17, 19, 25, 40):
            q = int(v * 10 ** (330 + nd))  # digits of v, cut: just below v; + 1: just above
            for m in (q, q + 1):
                near.append("%de-%d" % (m, 330 + nd))
                near.append("%s.%se-%d" % (str(m)[0], str(m)[1:], 330 + nd - len(str(m)) + 1))
    near += ["2.4703282292062327e-324", "2.4703282292062328e-324", "2.470328229206232720e-324",
             "2.470328229206232721e-324", "2.5e-324", "3e-324", "4.9e-324", "5e-324", "7.4e-324", "7.5e-324", "1e-323",
             "24703282292062328e-340", "123456789012345678e-340", "-2.4703282292062328e-324", "-2e-324", "1e-324",
             "2e-324", "9999999999999999999e-343", "1e-325", "1234567890123456789e-343", "2.2250738585072011e-308",
             "2.2250738585072014e-308", "0.00000000022250738585072014e-298"]
    sure = ["1e99999999999999999999", "-1e99999999999999999999", "1e+99999999999999999999", "1e-99999999999999999999",
            "-1e-99999999999999999999", "0.001e99999999999999999999", "1e100000", "1e-100000", "1e400", "1e-400",
            "-1e400", "-1e-400", "0e999999", "-0e999999", "0e99999999999999999999", "0e-99999999999999999999",
            "-0.0", "-0", "-0e5", "-.0", "+0.0", "0.0", "-0." + "0" * 400 + "e5", "1e310", "1e-345",
            "9999999999999999999e-344", "1" + "0" * 400, "0." + "0" * 400 + "1"]
    return tuple(s.encode() for s in near), tuple(s.encode() for s in sure)


OLD_TEST_STRINGS = ["abc", "", "1.2.3", "-", "1e", ".5", "5.", "+7", "0.000123", "00012"]
MALFORMED_MORE = ["inf", "nan", "Infinity", "-inf", "+nan", "INF", "NaN", "1_0", "0x10", "1e", "1e+", "1e-", ".", "+",
                  "+-1", "-+1", "--1", "1 2", "- 1", "1.2.3", "1e5.0", "1,5", "e", "E5", ".e5", "+.e5", "1e5e5", "1ee5",
                  "1 e5", "1e 5", "1. 5", "1-", "1+", "1e5+", "..5", "1..", "0x1p3", "1f", "1d5", "1.5x", "x1.5",
                  "1\x1c", "\x1c1", "1;", " ", " \t\n\v\f\r", "+ ", " - "]


@lru_cache(maxsize=None)
def malformed_corpus():
    """Mostly malformed spans (a few of the old strings are numbers: the oracle
    says which), shared by the f64 and the i64 tests."""
    toks = [s.encode("latin-1") for s in OLD_TEST_STRINGS + CM.BAD + MALFORMED_MORE]
    toks += [b"1\x002", b"\x001", b"1\x00", b"\x00", "١".encode(), "1٢".encode(), "１".encode(),
             b"\xa01", b"1\xa0", b"\xff", b"12\xb2"]
    return tuple(toks)


I64_FIXED = ["0", "1", "-1", "+1", "-0", "9223372036854775807", "-9223372036854775807", "-9223372036854775808",
             "+9223372036854775807", "9223372036854775808", "9999999999999999999", "-9223372036854775809",
             "-9999999999999999999", "+9223372036854775808", "9223372036854775806", "1000000000000000000",
             "0000000000000000001", "0000000000000000000", "-000000000000000001", "0009223372036854775",
             "00000000000000000001", "12345678901234567890", "09223372036854775807", "-09223372036854775808",
             "18446744073709551616", "18446744073709551617", "99999999999999999999", "1" + "0" * 30,
             "1.0", "1.", ".5", "-1.5", "1e3", "1E3", "1e0", "0.0", " 42 ", "\t-42\n", "\v7\f", "\r7"]


@lru_cache(maxsize=None)
def i64_corpus():
    rng = random.Random(505)
    toks = list(I64_FIXED) + list(CM.GOOD)
    for _ in range(2000):
        v = rng.randrange(-2**63, 2**63) >> rng.randrange(0, 64)
        s = "%d" % v
        r = rng.random()
        if r < 0.2 and v >= 0:
            s = "+" + s
        if r > 0.8:
            d = s.lstrip("-")
            s = s[:len(s) - len(d)] + "0" * rng.randrange(0, 21 - len(d)) + d  # up to 20 digit characters
        if 0.4 < r < 0.5:
            s = rng.choice(" \t\n\v\f\r") + s + rng.choice(" \t\n\v\f\r")
        toks.append(s)
    for _ in range(300):  # 19 digits on either side of 2^63
        v = 2**63 + rng.randrange(-10**6, 10**6) if rng.random() < 0.5 else rng.randrange(2**63, 10**19)
        toks.append(rng.choice(["", "-", "+"]) + str(v))
    return tuple(s.encode("latin-1") for s in toks) + malformed_corpus()


# -- the corpora hold what they claim (CPU) ------------------------------------------
def test_exact_corpus_precondition():
    toks = exact_corpus()
    assert len(toks) > 3000
    seen_m53 = seen_k22 = seen_cut = 0
    for t in toks:
        assert oracle_f64(t) is not None, t
        _neg, m, k = parts(t)
        assert m < 2**53 and -22 <= k <= 22, t
        v = value(t)
        assert Fraction(oracle_f64(t)) == Fraction(float(abs(v))) * (-1 if v < 0 else 1), t
        seen_m53 += m >= 2**53 - 16
        seen_k22 += abs(k) == 22
        written = t.strip(WS).lower().lstrip(b"+-").split(b"e")[0].replace(b".", b"").lstrip(b"0")
        seen_cut += len(written) > 19  # digits past the 19 the parser keeps (zeros here)
    assert seen_m53 > 50 and seen_k22 > 300 and seen_cut > 300
    for t in NEXT_TO_EXACT:
        _neg, m, k = parts(t)
        assert not (m < 2**53 and -22 <= k <= 22), t


def test_roundtrip_corpus_precondition():
    toks, src = roundtrip_corpus()
    assert len(toks) > 4000
    exps = set()
    for t, x in zip(toks, src):
        assert oracle_f64(t) == x and math.isfinite(x) and x != 0.0, t
        exps.add(math.frexp(x)[1] // 64)
    assert len(exps) >= 33  # binary exponents from -1074 to 1024 in steps of 64
    have = set(src)
    for x in (DBL_MIN, DBL_MAX, TINY, 2 * TINY, math.nextafter(DBL_MIN, 0), math.nextafter(DBL_MIN, 1),
              math.nextafter(DBL_MAX, 0)):
        assert x in have
    assert sum(1 for x in src if abs(x) < DBL_MIN) > 50  # subnormals
    assert sum(1 for x in src if abs(x) < 1e-290) > 400  # where pow(10, k) would be subnormal at 17 digits


def _sig_digits(t: bytes) -> int:
    return len(str(parts(t)[1]))


def _cut19(t: bytes) -> bytes:
    """The token with its significant digits past the 19th replaced by zeros."""
    neg, m, k = parts(t)
    s = str(m)
    return b"%s%se%d" % (b"-" if neg else b"", s[:19].encode(), k + len(s) - 19)


def test_long_corpus_precondition():
    toks, late = long_corpus()
    assert len(toks) >= 3000 and len(late) > 800
    for t in toks + late:
        assert oracle_f64(t) is not None, t
        _neg, _m, k = parts(t)
        assert 20 <= _sig_digits(t) <= 40, t
        assert -330 <= k + _sig_digits(t) - 1 <= 310, t
    assert any(oracle_f64(t) == 0.0 for t in toks) and any(math.isinf(oracle_f64(t)) for t in toks)
    # a correctly rounded parse of the first 19 digits alone gives another double
    decided = [t for t in late if oracle_f64(t) != oracle_f64(_cut19(t))]
    assert len(decided) > 150
    assert oracle_f64(b"9007199254740993." + b"0" * 10 + b"1") == 9007199254740994.0
    assert oracle_f64(_cut19(b"9007199254740993." + b"0" * 10 + b"1")) == 9007199254740992.0


def test_range_corpus_precondition():
    near, sure = range_corpus()
    top_inf = top_max = low0 = low1 = 0
    for t in near:
        x = oracle_f64(t)
        assert x is not None, t
        v = abs(value(t))
        if v > Fraction(10) ** 300:
            assert math.isinf(x) == (v >= T_INF), t
            top_inf += T_INF <= v < 2**1024
            top_max += DBL_MAX < v < T_INF
        elif v < Fraction(10) ** -300 and v <= Fraction(1, 2**1074):
            assert (x == 0.0) == (v <= Fraction(1, 2**1075)), t
            low0 += x == 0.0 and v > Fraction(1, 2**1076)
            low1 += abs(x) == TINY and v < Fraction(3, 2**1076)
    assert top_inf > 200 and top_max > 200 and low0 >= 8 and low1 >= 8
    for t in sure:
        x = oracle_f64(t)
        assert x == 0.0 or math.isinf(x), t
    assert math.copysign(1.0, oracle_f64(b"-0.0")) == -1.0 and math.copysign(1.0, oracle_f64(b"-1e-400")) == -1.0
    assert oracle_f64(b"1e99999999999999999999") == math.inf and oracle_f64(b"1e-99999999999999999999") == 0.0


def test_malformed_and_i64_corpus_precondition():
    bad = malformed_corpus()
    ok = {b".5", b"5.", b"+7", b"0.000123", b"00012"}
    for t in bad:
        assert (oracle_f64(t) is not None) == (t in ok), t
        assert (oracle_i64(t) is not None) == (t in (b"+7", b"00012")), t
    for s in ("inf", "nan", "Infinity", "1_0", "١", "１"):  # float() alone would take these
        float(s)
        assert oracle_f64(s.encode()) is None
    o = {t: oracle_i64(t) for t in i64_corpus()}
    assert o[b"9223372036854775807"] == 2**63 - 1 and o[b"-9223372036854775808"] == -2**63
    assert o[b"+9223372036854775807"] == 2**63 - 1 and o[b"-9223372036854775807"] == 1 - 2**63
    for t in (b"9223372036854775808", b"9999999999999999999", b"-9223372036854775809", b"00000000000000000001",
              b"12345678901234567890", b"1.0", b"1e3", b"18446744073709551617", b"09223372036854775807"):
        assert o[t] is None, t
    assert o[b"0000000000000000001"] == 1 and o[b"0009223372036854775"] == 9223372036854775
    good = [v for v in o.values() if v is not None]
    assert len(good) > 1500 and sum(v is None for v in o.values()) > 200
    assert sum(1 for t, v in o.items() if v is None and I64_RE.fullmatch(t)) > 100  # 19 digits, out of range


def test_pow5_table_is_correctly_rounded():
    """The committed table of the slow path (csrc/hip/text_pow5.h) holds the
    correctly rounded 5^k for every k it is indexed with."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "hip", "text_pow5.h")
    src = open(path).read()
    kmin, kmax = (int(x) for x in re.search(r"kPow5Min = (-?\d+), kPow5Max = (-?\d+);", src).groups())
    vals = [float.fromhex(h) for h in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", src.split("kPow5[", 1)[1])]
    assert (kmin, kmax) == (-343, 308) and len(vals) == kmax - kmin + 1
    # 10^19 * 10^(kmin - 1) < 2^-1075 and 10^(kmax + 1) > DBL_MAX: outside the table the result is 0 or inf
    assert Fraction(10) ** (19 + kmin - 1) < Fraction(1, 2**1075) and 10 ** (kmax + 1) > T_INF
    for k, v in zip(range(kmin, kmax + 1), vals):
        assert v == float(Fraction(5) ** k) and v >= DBL_MIN, k


# -- the CPU path against the oracle ------------------------------------------------
def _all_f64_tokens():
    return (exact_corpus() + roundtrip_corpus()[0] + sum(long_corpus(), ()) + sum(range_corpus(), ())
            + malformed_corpus())


def _expected_f64(toks):
    return np.array([math.nan if (x := oracle_f64(t)) is None else x for t in toks], dtype=np.float64)


def test_parse_f64_cpu_is_the_oracle():
    toks = _all_f64_tokens()
    t, st, ln = layout(toks)
    exp = _expected_f64(toks)
    got = TX.parse_f64(t, st, ln).numpy()
    d = distances(got, exp)
    assert not d.any(), [(toks[i], got[i], exp[i]) for i in np.flatnonzero(d)[:5]]
    with pytest.raises(ValueError):
        TX.parse_f64(t, st, ln, check=True)
    good = ~np.isnan(exp)
    TX.parse_f64(t, st[torch.from_numpy(good)], ln[torch.from_numpy(good)], check=True)
    # a missing field (start -1) and an empty span
    got = TX.parse_f64(t, torch.tensor([-1, 0, int(st[1])]), torch.tensor([3, 0, int(ln[1])], dtype=torch.int32))
    assert math.isnan(got[0]) and math.isnan(got[1]) and got[2] == exp[1]


def test_parse_i64_cpu_is_the_oracle():
    toks = i64_corpus()
    t, st, ln = layout(toks)
    exp = [oracle_i64(x) for x in toks]
    got = TX.parse_i64(t, st, ln).tolist()
    assert got == [0 if e is None else e for e in exp]
    with pytest.raises(ValueError):
        TX.parse_i64(t, st, ln, check=True)
    good = torch.tensor([e is not None for e in exp])
    TX.parse_i64(t, st[good], ln[good], check=True)
    for tok in (b"9223372036854775808", b"9999999999999999999", b"-9223372036854775809"):
        tt, s1, l1 = layout([tok])
        assert TX.parse_i64(tt, s1, l1).tolist() == [0]
        with pytest.raises(ValueError):
            TX.parse_i64(tt, s1, l1, check=True)
    got = TX.parse_i64(t, torch.tensor([-1, 0]), torch.tensor([3, 0], dtype=torch.int32))
    assert got.tolist() == [0, 0]


# -- the kernels ---------------------------------------------------------------------
def _launch(kind, text, starts, lens):
    """One launch of text_parse_f64_kernel / _i64_kernel: (values on the host, error word)."""
    from lua_mapreduce_1_amd.ops import _hip
    d = text.device
    st = starts.to(d, torch.int64).contiguous()
    ln = lens.to(d, torch.int32).contiguous()
    out = torch.full((st.numel(),), 77, dtype=torch.float64 if kind == "f64" else torch.int64, device=d)
    err = torch.zeros(1, dtype=torch.int32, device=d)
    _hip.call("mr_text_parse_" + kind, _hip.ptr(text), _hip.ptr(st), _hip.ptr(ln), st.numel(), _hip.ptr(out),
              _hip.ptr(err), _hip.stream(d))
    return out.cpu(), int(err.item())


def _gpu_f64(gpu, toks):
    t, st, ln = layout(toks)
    got, err = _launch("f64", t.to(gpu), st, ln)
    return got.numpy(), err


def _report(name, toks, got, exp, bound):
    d = distances(got, exp)
    worst = int(d.max())
    print("%s: %d tokens, worst distance %d, %.1f %% at distance 0" % (name, len(toks), worst, 100.0 * (d == 0).mean()))
    far = np.flatnonzero(d > bound)
    assert far.size == 0, (name, [(toks[i], float(got[i]), float(exp[i]), int(d[i])) for i in far[:8]])
    return worst


@pytest.mark.gpu
def test_f64_exact_class_gpu(gpu):
    toks = exact_corpus()
    got, err = _gpu_f64(gpu, toks)
    assert err == 0
    _report("exact", toks, got, _expected_f64(toks), 0)


@pytest.mark.gpu
def test_f64_distance_classes_gpu(gpu):
    """Round-trip, long and range-end tokens: within B of float(); the worst
    distance of each class is printed (and recorded in the module docstring)."""
    rt = roundtrip_corpus()[0]
    lg, late = long_corpus()
    near, sure = range_corpus()
    worst = {}
    for name, toks, bound in (("round-trip", rt, B), ("long", lg + late, B), ("range ends", near, B),
                              ("beyond doubt", sure, 0)):
        got, err = _gpu_f64(gpu, toks)
        assert err == 0, name
        worst[name] = _report(name, toks, got, _expected_f64(toks), bound)
    assert max(worst.values()) <= B


@pytest.mark.gpu
def test_f64_malformed_gpu(gpu):
    toks = malformed_corpus()
    exp = _expected_f64(toks)
    got, err = _gpu_f64(gpu, toks)
    assert err == 1
    _report("malformed", toks, got, exp, 0)
    t, st, ln = layout(toks)
    dt = t.to(gpu)
    for i in np.flatnonzero(np.isnan(exp)):  # each alone sets the word
        g, e = _launch("f64", dt, st[i:i + 1], ln[i:i + 1])
        assert e == 1 and math.isnan(g[0]), toks[i]
    # a missing field (start -1, whatever its length) and an empty span
    g, e = _launch("f64", dt, torch.tensor([-1, -1, 0]), torch.tensor([3, 0, 0]))
    assert e == 1 and all(math.isnan(x) for x in g.tolist())
    with pytest.raises(ValueError):
        TX.parse_f64(dt, st.to(gpu), ln.to(gpu), check=True)
    ok = torch.from_numpy(~np.isnan(exp))
    assert ok.sum() == 5
    TX.parse_f64(dt, st[ok].to(gpu), ln[ok].to(gpu), check=True)


@pytest.mark.gpu
def test_i64_gpu(gpu):
    toks = i64_corpus()
    exp = [oracle_i64(x) for x in toks]
    t, st, ln = layout(toks)
    dt = t.to(gpu)
    got, err = _launch("i64", dt, st, ln)
    want = [0 if e is None else e for e in exp]
    wrong = [(toks[i], g, w) for i, (g, w) in enumerate(zip(got.tolist(), want)) if g != w]
    assert not wrong, wrong[:8]
    assert err == 1
    good = torch.tensor([e is not None for e in exp])
    g, e = _launch("i64", dt, st[good], ln[good])
    assert e == 0 and g.tolist() == [x for x in exp if x is not None]
    assert torch.equal(TX.parse_i64(dt, st[good].to(gpu), ln[good].to(gpu), check=True).cpu(), g)
    for i in np.flatnonzero(~good.numpy()):  # each alone: 0 and the error word
        g, e = _launch("i64", dt, st[i:i + 1], ln[i:i + 1])
        assert e == 1 and g.tolist() == [0], toks[i]
    with pytest.raises(ValueError):
        TX.parse_i64(dt, st.to(gpu), ln.to(gpu), check=True)
    g, e = _launch("i64", dt, torch.tensor([-1, 0]), torch.tensor([3, 0]))
    assert e == 1 and g.tolist() == [0, 0]


GRID_SPAN = 8192 * 256  # spans one trip of the kernels' grid-stride loop covers


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 255, 256, 257, GRID_SPAN + 1])
def test_span_counts_and_error_word_gpu(gpu, m):
    """Span counts around a block and past the grid-stride limit (the last
    span alone takes the loop's second trip): every value, the error word 0
    for an all-good launch, 1 when only the last span is bad."""
    text = torch.frombuffer(bytearray(b"7;" * (m - 1) + b"42;x;"), dtype=torch.uint8).to(gpu)
    st = torch.arange(m, dtype=torch.int64) * 2
    ln = torch.ones(m, dtype=torch.int32)
    ln[-1] = 2
    exp = torch.full((m,), 7, dtype=torch.int64)
    exp[-1] = 42
    for kind in ("f64", "i64"):
        got, err = _launch(kind, text, st, ln)
        assert err == 0 and torch.equal(got.to(torch.int64), exp), kind
    st[-1] += 3  # the "x"
    ln[-1] = 1
    got, err = _launch("f64", text, st, ln)
    assert err == 1 and math.isnan(got[-1]) and torch.equal(got[:-1].to(torch.int64), exp[:-1])
    got, err = _launch("i64", text, st, ln)
    assert err == 1 and got[-1] == 0 and torch.equal(got[:-1], exp[:-1])
    if m <= 257:
        with pytest.raises(ValueError):
            TX.parse_f64(text, st.to(gpu), ln.to(gpu), check=True)
        with pytest.raises(ValueError):
            TX.parse_i64(text, st.to(gpu), ln.to(gpu), check=True)


@pytest.mark.gpu
def test_span_order_views_and_overlap_gpu(gpu):
    """Unaligned views of the text, starts in descending order and spans that
    overlap: each span is parsed on its own bytes."""
    toks = (exact_corpus()[:400] + roundtrip_corpus()[0][:400] + long_corpus()[0][:200] + malformed_corpus())
    exp = _expected_f64(toks)
    t, st, ln = layout(toks)
    ref, err0 = _launch("f64", t.to(gpu), st, ln)
    assert _report("mixed", toks, ref.numpy(), exp, B) <= B
    for off in (1, 3):
        view = torch.cat([torch.full((off,), ord("9"), dtype=torch.uint8), t]).to(gpu)[off:]
        got, err = _launch("f64", view, st, ln)
        assert err == err0 == 1 and not distances(got.numpy(), ref.numpy()).any(), off
    got, err = _launch("f64", t.to(gpu), st.flip(0), ln.flip(0))
    assert not distances(got.numpy(), ref.flip(0).numpy()).any()
    ints = [x for x in i64_corpus()[:600]]
    ti, si, li = layout(ints)
    gi, _ = _launch("i64", ti.to(gpu), si.flip(0), li.flip(0))
    assert gi.tolist() == [oracle_i64(x) or 0 for x in reversed(ints)]
    gi, _ = _launch("i64", torch.cat([torch.full((3,), ord("9"), dtype=torch.uint8), ti]).to(gpu)[3:], si, li)
    assert gi.tolist() == [oracle_i64(x) or 0 for x in ints]
    # every sub-span of one token, all overlapping
    tok = b"-12.5e+3 "
    spans = [(a, n) for a in range(len(tok)) for n in range(0, len(tok) - a + 1)]
    text = torch.frombuffer(bytearray(tok), dtype=torch.uint8).to(gpu)
    s2 = torch.tensor([a for a, _ in spans])
    l2 = torch.tensor([n for _, n in spans])
    got, err = _launch("f64", text, s2, l2)
    assert err == 1 and not distances(got.numpy(), _expected_f64([tok[a:a + n] for a, n in spans])).any()
    gi, err = _launch("i64", text, s2, l2)
    assert gi.tolist() == [oracle_i64(tok[a:a + n]) or 0 for a, n in spans]


# -- the fused CSV fold ----------------------------------------------------------------
TILE = 8192  # CV_TILE of csrc/hip/generic.hip


@lru_cache(maxsize=None)
def csv_text():
    """Lines ``k<i>,<token>`` with a key of their own, laid out so that at
    the multiples of TILE a value field sits: ending on the tile's last byte,
    straddling the tile end, or in a line whose first byte is the tile's last
    (every other line lies wholly inside a tile); each before ``\\n`` and
    before ``\\r\\n``, with slow-path, malformed and other tokens in turn; the
    last line of the text has no newline.  Lines without a separator pad the
    layout (rows without a value field: dropped).

    -> (bytes, rows [(key, field start, field length)])."""
    pool = (list(exact_corpus()[:900:3]) + list(roundtrip_corpus()[0][::9]) + list(long_corpus()[0][::20])
            + list(long_corpus()[1][::40]) + [t for t in range_corpus()[0] if len(t) < 60][::4]
            + [t for t in range_corpus()[1] if len(t) < 60] + list(malformed_corpus()))
    # (zeros stay out: the sign of a zero in a min / max fold is not this test's subject)
    pool = [t for t in pool if b"\n" not in t and b"," not in t and oracle_f64(t) != 0.0]
    slow = [t for t in pool if oracle_f64(t) is not None and parts(t)[1] >= 2**53 and len(t) > 12]
    bad = [t for t in pool if oracle_f64(t) is None and len(t) > 1 and b"\r" not in t]
    fast = [t for t in pool if oracle_f64(t) is not None and parts(t)[1] < 2**53 and 2 < len(t) < 12
            and t.strip(WS) == t]
    assert len(slow) > 50 and len(bad) > 30 and len(fast) > 50
    buf = bytearray()
    rows, seen = [], set()

    def line(tok, eol, where=None, edge=0):
        """Append a line; with ``where``, after a pad line that puts the value
        field's end ("end"), a byte inside it ("mid") or the line's first
        byte + 1 ("start") on the offset ``edge``."""
        key = b"k%d" % len(rows)
        if where is not None:
            at = {"end": len(key) + 1 + len(tok), "mid": len(key) + 1 + len(tok) // 2, "start": 1}[where]
            n = edge - at - len(buf) - 1
            assert n >= 0
            buf.extend(b"#" * n + b"\n")
        fs = len(buf) + len(key) + 1
        rows.append((key, fs, len(tok)))
        buf.extend(key + b"," + tok + eol)
        return fs

    kinds = [(w, e) for w in ("end", "mid", "start") for e in (b"\n", b"\r\n")]
    j = 0
    for b in range(1, 4 * len(kinds) + 1):
        edge = b * TILE
        for _ in range(110):
            line(pool[j % len(pool)], b"\r\n" if j % 7 == 0 else b"\n")
            j += 1
        where, eol = kinds[b % len(kinds)]
        cls = (b // len(kinds)) % 3
        tok = (slow, bad, fast)[cls][b % 29]
        fs = line(tok, eol, where, edge)
        seen.add((where, eol, cls))
        if where == "end":      # the field's last byte is the tile's last
            assert fs + len(tok) == edge
        elif where == "mid":    # the field straddles the tile end
            assert fs < edge < fs + len(tok)
        else:                   # the line's first byte is the tile's last
            assert fs - len(rows[-1][0]) - 1 == edge - 1
    line(slow[3], b"")  # the end of the text closes the last field
    assert {s[:2] for s in seen} == set(kinds) and {(s[0], s[2]) for s in seen} >= {(w, 0) for w, _ in kinds}
    return bytes(buf), tuple(rows)


def _csv_oracle(data: bytes):
    """Rows of the text by the definition: lines end at \\n, a trailing \\r is
    dropped, field 0 is the key (not empty), field 1 a well-formed number."""
    keep = {}
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for ln in lines:
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        f = ln.split(b",")
        if len(f) >= 2 and f[0] and oracle_f64(f[1]) is not None:
            assert f[0] not in keep
            keep[f[0]] = f[1]
    return keep


def test_csv_text_layout():
    data, rows = csv_text()
    keep = _csv_oracle(data)
    assert 2000 < len(rows) < 6000 and 0.7 * len(rows) < len(keep) < len(rows)
    for key, fs, fl in rows:
        assert data[fs - len(key) - 1:fs] == key + b"," and data[fs + fl:fs + fl + 1] in (b"\n", b"\r", b"")
    assert not data.endswith(b"\n")


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [0, 4], ids=["auto", "4tiles"])
@pytest.mark.parametrize("shift", [0, 1])
def test_csv_fold_parses_like_parse_f64_gpu(gpu, shift, tiles):
    """mr_csv_fold over one row per key, the text at offset 0 and 1 of its
    buffer (16-byte loads / byte loads), one and four tiles a block: the keys kept are the oracle's rows,
    min and max of each key are bit for bit what TX.parse_f64 gives on the
    GPU for the same span, rows_out counts them, and TX.csv_rows (the chain
    the fused kernel is specified by) yields the same rows."""
    from lua_mapreduce_1_amd import ops
    from lua_mapreduce_1_amd.ops import _hip
    from lua_mapreduce_1_amd.ops import agg as A
    from lua_mapreduce_1_amd.utils.config import TUNABLES
    data, rows = csv_text()
    keep = _csv_oracle(data)
    text = torch.frombuffer(bytearray(b"\n" * shift + data), dtype=torch.uint8).to(gpu)[shift:]
    st = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    ln = torch.tensor([r[2] for r in rows], dtype=torch.int32)
    parsed, _ = _launch("f64", text, st, ln)
    by_key = {r[0]: v for r, v in zip(rows, bits(parsed.numpy()).tolist())}
    exp = _expected_f64([data[r[1]:r[1] + r[2]] for r in rows])
    assert _report("csv fields", [r[0] for r in rows], parsed.numpy(), exp, B) <= B
    assert set(keep) == {r[0] for r, x in zip(rows, exp) if not math.isnan(x)}

    t = A.AggTable(1 << 14, gpu, [("f64", "min", 0), ("f64", "max", 0), ("i64", "sum", None)])
    t.src = text
    nrows = torch.zeros(1, dtype=torch.int64, device=gpu)
    assert _hip.lib().mr_csv_set_config(tiles, TUNABLES.csv_mode) == 0
    try:
        t.insert_csv(text, 0, 0, (1,), ord(","), nrows)
        torch.cuda.synchronize()
    finally:
        _hip.lib().mr_csv_set_config(TUNABLES.csv_tiles, TUNABLES.csv_mode)
    _slot, hi, lo, rep, cols = t.compact()
    keys = ops.key_bytes_list(hi.cpu(), lo.cpu(), rep.cpu(), text.cpu())
    assert len(keys) == len(set(keys)) and set(keys) == set(keep)
    assert int(nrows.item()) == len(keep)
    lo_, hi_, cnt = (c.cpu() for c in cols)
    assert cnt.tolist() == [1] * len(keys)
    want = [by_key[k] for k in keys]
    assert bits(lo_.numpy()).tolist() == want and bits(hi_.numpy()).tolist() == want

    ks, kl, (x,) = TX.csv_rows(text, 0, (1,), ",")
    ks, kl, x = ks.cpu().tolist(), kl.cpu().tolist(), bits(x.cpu().numpy()).tolist()
    chain = {data[s:s + n]: v for s, n, v in zip(ks, kl, x) if n > 0}
    assert chain == {k: by_key[k] for k in keep}

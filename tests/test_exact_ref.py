"""tests/exact_ref.py checked on the CPU against independent arithmetic (mpmath at 200 bits,
fractions.Fraction, the host's IEEE operations), glibc's pow measured against it, and the kernels'
double-double powering (rt_math.inc: dd_sqr / dd_mul / pow_bin) restated with an exact fma to
show which mistakes tests/test_gpu_math_exact.py catches."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_ref as X

STRUCTURED_N = (1, 2, 3, 4, 5, 7, 20, 21, 63, 64, 255, 256, 511, 512, 513, 768, 1000, 1023, 1024)
EDGE_X = (0.0, 2.0 ** -1074, 2.0 ** -537, 0.5, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -20)


def _operands(rnd, count):
    """(x, n): uniform x with random n, and x = 2**(t/n) aimed at results over [2**-1080, 1]."""
    out = []
    for i in range(count):
        n = rnd.choice(STRUCTURED_N) if i % 3 == 0 else rnd.randint(0, 1024)
        if i % 2 == 0 or n == 0:
            x = rnd.random()
        else:
            x = 2.0 ** (-1080.0 * rnd.random() / n)
        out.append((x, n))
    out += [(x, n) for x in EDGE_X for n in STRUCTURED_N + (0,)]
    return out


def test_exact_pow_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    rnd = random.Random(0xE1)
    with mpmath.workprec(200):
        for x, n in _operands(rnd, 1500):
            got = X.exact_pow(x, n)
            p = mpmath.mpf(x) ** n  # 200 bits: relative error 2**-199
            # the correctly rounded value is within half a unit of the true one: bracket it with
            # the neighbours of `got` (exact in 200 bits)
            if got == 0.0:
                assert p <= mpmath.mpf(2) ** -1075, (x, n)
                continue
            lo, hi = math.nextafter(got, -math.inf), math.nextafter(got, math.inf)
            half_lo, half_hi = (mpmath.mpf(got) - mpmath.mpf(lo)) / 2, (mpmath.mpf(hi) - mpmath.mpf(got)) / 2
            slack = p * mpmath.mpf(2) ** -190
            assert mpmath.mpf(got) - half_lo - slack <= p <= mpmath.mpf(got) + half_hi + slack, (x, n, got)


def test_exact_pow_against_fractions():
    rnd = random.Random(0xE2)
    ops = _operands(rnd, 3000)
    for x, n in ops:
        want = float(Fraction(x) ** n)  # int / int true division rounds correctly, subnormals included
        assert X.exact_pow(x, n) == want, (x, n)
    xs = np.array([x for x, _ in ops])
    ns = np.array([n for _, n in ops])
    assert np.array_equal(X.exact_pow_array(xs, ns), np.array([X.exact_pow(x, n) for x, n in ops]))


def test_exact_pow_half_against_fractions():
    """x**0.5 is the host's (correctly rounded) sqrt; x**2.5 lies between the squares of the midpoints
    to its result's neighbours, exactly (fractions), down into the subnormal results."""
    rnd = random.Random(0xE7)
    xs = [rnd.random() for _ in range(1500)] + [2.0 ** (-430.0 * rnd.random()) for _ in range(1500)] + list(EDGE_X)
    for x in xs:
        assert X.exact_pow_half(x, 1) == math.sqrt(x) == X.exact_sqrt(x), x
        got = X.exact_pow_half(x, 5)
        true_sq = Fraction(x) ** 5
        if got == 0.0:
            assert true_sq <= Fraction(2.0 ** -1074) ** 2 / 4, x
            continue
        lo = (Fraction(got) + Fraction(math.nextafter(got, 0.0))) / 2
        hi = (Fraction(got) + Fraction(math.nextafter(got, math.inf))) / 2
        assert lo * lo <= true_sq <= hi * hi, (x, got)
    assert X.exact_pow_half(4.0, 5) == 32.0 and X.exact_pow_half(0.25, 1) == 0.5 and X.exact_pow_half(1.0, 5) == 1.0
    with pytest.raises(ValueError):
        X.exact_pow_half(2.0, 4)


def test_exact_pow_edges():
    assert X.exact_pow(0.0, 0) == 1.0 and X.exact_pow(0.0, 5) == 0.0 and X.exact_pow(1.0, 1024) == 1.0
    assert X.exact_pow(0.5, 1074) == 2.0 ** -1074
    assert X.exact_pow(0.5, 1075) == 0.0                     # the tie with 0 goes to even
    assert X.exact_pow(math.nextafter(0.5, 1.0), 1075) == 2.0 ** -1074
    assert X.exact_pow(2.0 ** -537, 2) == 2.0 ** -1074
    assert X.exact_pow(2.0 ** -1074, 1) == 2.0 ** -1074 and X.exact_pow(2.0 ** -1074, 2) == 0.0
    assert X.exact_pow(3.0, 2) == 9.0 and X.exact_pow(2.0, 1024) == math.inf
    assert X.exact_pow(1.0 + 2.0 ** -52, 2) == 1.0 + 2.0 ** -51   # 1 + 2^-51 + 2^-104 rounds down
    with pytest.raises(ValueError):
        X.exact_pow(-1.0, 2)


def glibc_pow_rates(exponents, per_exponent, seed):
    """Fraction of uniform x in [0, 1) with math.pow(x, n) != exact_pow(x, n), per exponent, over the
    calls whose exact result is a normal number; and the largest distance seen, in ulps."""
    rnd = random.Random(seed)
    rates, worst = {}, 0
    for n in exponents:
        bad = tot = 0
        for _ in range(per_exponent):
            x = rnd.random()
            want = X.exact_pow(x, n)
            d = int(X.ulps_apart(math.pow(x, n), want))
            worst = max(worst, d)
            if want >= 2.0 ** -1022:
                tot += 1
                bad += d != 0
        rates[n] = bad / max(tot, 1)
    return rates, worst


def test_glibc_pow_within_one_ulp_and_its_rate():
    """The host libm's pow (the oracle's, and BEAM's math:pow/2) is never more than 1 ulp from the
    correctly rounded value; the rate at which it differs is printed per exponent (the scene
    bounds of tests/test_gpu_math_exact.py are built on it)."""
    ns = (2, 3, 7, 1024, 5, 64, 255, 1023, 1, 4, 20)
    rates, worst = glibc_pow_rates(ns, 4000, 0xE3)
    for n in ns:
        print(f"glibc pow(x, {n}) != correctly rounded: {rates[n]:.5f} of 4000 uniform x")
    print(f"glibc pow: mean rate {sum(rates.values()) / len(rates):.5f}, largest distance {worst} ulp")
    assert worst <= 1
    rnd = random.Random(0xE4)
    for x, n in _operands(rnd, 3000):
        assert X.ulps_apart(math.pow(x, n), X.exact_pow(x, n)) <= 1, (x, n)
    # x and x*x are exact / correctly rounded in any libm
    assert rates[1] == 0.0


def test_host_sqrt_and_division_are_correctly_rounded():
    rnd = random.Random(0xE5)
    for _ in range(3000):
        x = math.ldexp(1.0 + rnd.random(), rnd.randint(-1070, 1020))
        assert X.exact_sqrt(x) == math.sqrt(x) == float(X.ref_sqrt(x)), x
        a = math.ldexp(1.0 + rnd.random(), rnd.randint(-300, 300))
        b = math.ldexp(1.0 + rnd.random(), rnd.randint(-400, 400))
        assert X.exact_div(a, b) == a / b == float(X.ref_div(a, b)) == float(Fraction(a) / Fraction(b)), (a, b)
    for x in (0.0, 2.0 ** -1074, 2.0 ** -768, 2.0 ** -767, 2.0 ** 1000, 2.0 ** 1001, 4.0, 2.0, 3.0 * 2.0 ** -1074):
        assert X.exact_sqrt(x) == math.sqrt(x), x
    for a, n in ((7, 3), (1 << 43, 1048575), (2147483647, 97), (0, 5), (96, 97), (97, 97)):
        assert X.exact_div(float(a), float(n)) == a / n
    assert list(X.ref_floordiv([0, 96, 97, 98, 2147483647], 97)) == [0, 0, 1, 1, 2147483647 // 97]


def test_ref_normalize3():
    v = np.array([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0], [1e-170, 0.0, 0.0], [1e200, 1e200, 0.0], [1.0, 2.0, 3.0]])
    u = X.ref_normalize3(v)
    assert np.array_equal(u[0], [3.0 * (1.0 / 5.0), 0.0, 4.0 * (1.0 / 5.0)])
    assert np.array_equal(u[1], [0.0, 0.0, 0.0])
    assert np.array_equal(u[2], [0.0, 0.0, 0.0])          # m2 underflows to 0: Mag == 0
    assert np.array_equal(u[3], [0.0, 0.0, 0.0])          # m2 overflows: 1/inf = 0
    m = math.sqrt(1.0 * 1.0 + 2.0 * 2.0 + 3.0 * 3.0)
    assert np.array_equal(u[4], [1.0 * (1.0 / m), 2.0 * (1.0 / m), 3.0 * (1.0 / m)])


# ---- the kernels' powering, restated with an exact fma ------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding


def _dd_sqr(h, l):
    p = h * h
    return p, _fma(h + h, l, _fma(h, h, -p))


def _dd_mul(ah, al, bh, bl, plain=False):
    p = ah * bh
    if plain:  # the mistake C1 must catch: the product's rounding error is dropped
        return p, 0.0
    return p, _fma(al, bh, _fma(ah, bl, _fma(ah, bh, -p)))


def _pow_bin(x, n, plain=False):
    bh, bl = x, 0.0
    while not n & 1:
        bh, bl = _dd_sqr(bh, bl)
        n >>= 1
    rh, rl = bh, bl
    n >>= 1
    while n:
        bh, bl = _dd_sqr(bh, bl)
        if n & 1:
            rh, rl = _dd_mul(rh, rl, bh, bl, plain)
        n >>= 1
    return rh + rl


def test_double_double_powering_restated():
    """pow_bin as the kernels compute it equals exact_pow wherever the result is >= 2**-969 or 0; below
    2**-969 the pairs' low parts are subnormal and the products' error terms are no longer exact:
    within one unit there, and some do differ (the GPU test's two lower bands).  With dd_mul
    replaced by a plain product the normal range fails: the mistake the GPU test's normal band is
    there to catch."""
    rnd = random.Random(0xE6)
    ops = [(x, n) for x, n in _operands(rnd, 1500) if n >= 1]
    ops += [(2.0 ** (-t / n), n) for n in (3, 21, 255, 513, 1000, 1023, 1024)
            for t in [rnd.uniform(969.0, 1077.0) for _ in range(150)]]
    ops += [(math.ldexp(1.0 + rnd.random(), -rnd.randint(1, 1074)), rnd.randint(1, 8)) for _ in range(400)]
    ops += [(math.ldexp(rnd.randint(1, 1 << 52), -1074), n) for n in (1, 2, 3) for _ in range(20)]  # subnormal x
    bad_plain = bad_tiny = 0
    for x, n in ops:
        want = X.exact_pow(x, n)
        got = _pow_bin(x, n)
        if want >= 2.0 ** -969 or want == 0.0:
            assert got == want, (x, n)
            bad_plain += _pow_bin(x, n, plain=True) != want
        else:
            assert X.ulps_apart(got, want) <= 1, (x, n)
            bad_tiny += got != want
    assert bad_plain > 50 and bad_tiny > 10

"""Exact references for the kernels' arithmetic primitives (rt_math.inc: pow_libm, sqrt_x,
div_n, normalize3, div_dim, idiv_dim), for tests/test_gpu_math_exact.py.  Not part of the product.

* exact_pow / exact_sqrt / exact_div: Python integers only.  The operand's mantissa is taken to
  the power (or its integer square root / quotient is formed) exactly and rounded ONCE to
  binary64, to nearest, ties to even, with gradual underflow — the correctly rounded result by
  construction.  tests/test_exact_ref.py checks them against mpmath and fractions.Fraction.
* ref_sqrt / ref_div / ref_normalize3 / ref_floordiv: the same operations with numpy (IEEE
  binary64 sqrt and division on the host are correctly rounded; test_exact_ref.py checks that
  against the integer forms), normalize3 in the reference's operation order
  (vector_normalize/1, raytracer.erl:554-560), every operation rounded separately.
"""
import math

import numpy as np

MANT = 53
EMIN = -1074  # exponent of the smallest subnormal's unit


def _decompose(x):
    """A finite x > 0 as (m, e) with x == m * 2**e, m odd."""
    f, e = math.frexp(x)
    m = int(f * (1 << MANT))  # exact: f has at most 53 significant bits
    e -= MANT
    tz = (m & -m).bit_length() - 1
    return m >> tz, e + tz


def round_scaled(M, E, sticky=False):
    """M * 2**E (M a non-negative int; plus a positive amount below one unit of M when
    `sticky`), rounded once to binary64: nearest, ties to even, subnormals, 0 and inf."""
    if M == 0:
        return 0.0
    if sticky:  # one more bit carries "a little more than M": it lies below any rounding position
        assert M.bit_length() > MANT + 2
        M, E = (M << 1) | 1, E - 1
    top = M.bit_length() + E                # 2**(top-1) <= value < 2**top
    q_exp = max(top - MANT, EMIN)           # the exponent of the result's unit in the last place
    shift = q_exp - E
    if shift <= 0:
        q = M << -shift
    elif shift > M.bit_length() + 1:        # below half of the smallest subnormal
        return 0.0
    else:
        q, rem, half = M >> shift, M & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
    try:
        return math.ldexp(q, q_exp)         # q <= 2**53: exact
    except OverflowError:
        return math.inf


def exact_pow(x, n, _cache=None):
    """The correctly rounded binary64 value of x**n for a finite x >= 0 and an integer n >= 0
    (x**0 = 1 for every x, as math:pow/2 and C's pow)."""
    n = int(n)
    if n < 0 or not (x >= 0.0) or math.isinf(x):
        raise ValueError(f"exact_pow({x!r}, {n!r})")
    if n == 0:
        return 1.0
    if x == 0.0:
        return 0.0
    m, e = _decompose(x)
    if m == 1:
        return round_scaled(1, e * n)
    # far below the smallest subnormal: skip the big power (x < 2**(e + bits))
    if (e + m.bit_length()) * n < EMIN - 2:
        return 0.0
    if _cache is not None:
        key = (m, n)
        M = _cache.get(key)
        if M is None:
            M = _cache[key] = m ** n
    else:
        M = m ** n
    return round_scaled(M, e * n)


def exact_pow_array(xs, ns):
    """exact_pow elementwise (ns a scalar or an array), as a float64 array."""
    xs = np.asarray(xs, dtype=np.float64)
    ns = np.broadcast_to(np.asarray(ns), xs.shape)
    cache = {}
    return np.array([exact_pow(float(x), int(n), cache) for x, n in zip(xs.ravel(), ns.ravel())],
                    dtype=np.float64).reshape(xs.shape)


def exact_sqrt(x):
    """The correctly rounded sqrt of a finite x >= 0 (integer square root plus a sticky bit)."""
    if x == 0.0:
        return 0.0
    m, e = _decompose(x)
    k = 2 * (MANT + 6)                      # m * 2**k >= 2**118: the root has at least 59 bits
    if (e - k) & 1:                         # the exponent left over must be even
        k += 1
    M = m << k
    r = math.isqrt(M)
    return round_scaled(r, (e - k) // 2, sticky=r * r != M)


def exact_pow_half(x, k):
    """The correctly rounded x**(k/2) for a finite x >= 0 and an odd k >= 1 (k = 1: sqrt(x); k = 5:
    x^2 sqrt(x) = x**2.5): the integer square root of m^k scaled, plus a sticky bit."""
    k = int(k)
    if k < 1 or not (k & 1) or not (x >= 0.0) or math.isinf(x):
        raise ValueError(f"exact_pow_half({x!r}, {k!r})")
    if x == 0.0:
        return 0.0
    m, e = _decompose(x)
    M, E = m ** k, e * k
    s = 2 * (MANT + 6)                      # M * 2**s >= 2**118: the root has at least 59 bits
    if (E - s) & 1:                         # the exponent left over must be even
        s += 1
    M <<= s
    r = math.isqrt(M)
    return round_scaled(r, (E - s) // 2, sticky=r * r != M)


def exact_div(a, b):
    """The correctly rounded a / b for finite a >= 0, b > 0 (integer quotient plus a sticky bit)."""
    if a == 0.0:
        return 0.0
    ma, ea = _decompose(a)
    mb, eb = _decompose(b)
    k = mb.bit_length() + MANT + 8
    q, rem = divmod(ma << k, mb)            # q >= 2**(MANT + 7)
    return round_scaled(q, ea - eb - k, sticky=rem != 0)


def ulps_apart(a, b):
    """|a - b| in units of the binary64 grid (adjacent non-negative doubles are 1 apart; in
    the subnormal band one unit is 2**-1074)."""
    ia = np.asarray(a, dtype=np.float64).view(np.int64)
    ib = np.asarray(b, dtype=np.float64).view(np.int64)
    return np.abs(ia - ib)


# ---- numpy restatements (every operation rounded separately; no contraction) --------------
def ref_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, dtype=np.float64))


def ref_div(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)


def ref_normalize3(v):
    """vector_normalize/1 (raytracer.erl:554-560) on an (n, 3) array: Mag = sqrt(X*X + Y*Y + Z*Z),
    (0, 0, 0) if Mag == 0, else each component times 1/Mag."""
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        m2 = x * x + y * y + z * z
        mag = np.sqrt(m2)
        s = 1.0 / mag
        out = np.stack([x * s, y * s, z * s], axis=1)
    out[mag == 0] = 0.0
    return out


def ref_floordiv(a, n):
    """floor(a / n) for non-negative integers, in Python integers."""
    n = int(n)
    return np.array([int(t) // n for t in np.asarray(a).ravel()], dtype=np.int64)

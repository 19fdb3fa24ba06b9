"""The kernels' arithmetic primitives (rt_math.inc: pow_libm / pow_bin, sqrt_x, div_n, normalize3,
div_dim, idiv_dim) run on the GPU through rt_eval_math, one operand per work-item in array order
(64 consecutive elements are one wave), against exact references (tests/exact_ref.py: Python
integers rounded once; the host's IEEE sqrt and division), bit for bit.  Frames cannot judge
these: the oracle's pow is glibc's, which is not correctly rounded, so frame tests bound a count.
"""
import ctypes

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import scenes
from eraytracer_amd.raytracer import render
from tests import exact_ref as X
from tests.test_gpu_fullsize import _compare

pytestmark = pytest.mark.gpu

STRUCTURED_N = (1, 2, 3, 4, 5, 7, 20, 21, 63, 64, 255, 256, 511, 512, 513, 768, 1000, 1023, 1024)
EDGE_X = (0.0, 2.0 ** -1074, 2.0 ** -537, 0.5, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -20)
# Results below 2**-969 are within one unit in the last place (2**-1074 in the subnormal band) of the
# correctly rounded value, not always equal to it (rt_math.inc, above dd_sqr; DESIGN.md section 3:
# the pairs' low parts are subnormal there).  Measured on MI355X, the same in all three layouts: 42
# of 2,168 operands in [2**-1022, 2**-969) and 112 of 2,019 subnormal ones differ, each by 1.
TINY_BAND_ULPS = 1


def ev(op, a, b=None, act=None, dim=0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.size // 3 if op == N.RT_EVAL_NORMALIZE3 else a.size
    out = np.full(a.shape, np.nan)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.shape == a.shape
    if act is not None:
        act = np.ascontiguousarray(act, dtype=np.uint8)
        assert act.size == n
    N.check(N.lib().rt_eval_math(0, op, n, a.ctypes.data, None if b is None else b.ctypes.data,
                                 None if act is None else act.ctypes.data, dim, out.ctypes.data), "rt_eval_math")
    return out


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def assert_bits(got, want, what, operands):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ; first at {bad[:5]}: operands "
                           f"{[tuple(float(o.ravel()[i]).hex() for o in operands) for i in bad[:5]]}, got "
                           f"{[float(got.ravel()[i]).hex() for i in bad[:5]]}, want "
                           f"{[float(want.ravel()[i]).hex() for i in bad[:5]]}")


# ---- 1. pow, integer path ------------------------------------------------------------------
@pytest.fixture(scope="module")
def pow_set():
    """Waves of 64 operands with one exponent each: every n in 0..1024 (16 uniform x in [0, 1), 16
    x = 2**(t/n) aiming the result log-uniformly over [2**-1080, 1]; the 32 fill a wave twice), and
    two more waves for each structured exponent (the edge x, 60 uniform, 60 aimed).  The exact
    results are computed once here (about 35,000 exact_pow calls)."""
    rng = np.random.default_rng(0x5EED9)
    xs, ns = [], []
    for n in range(1025):
        x = np.concatenate([rng.random(16), 2.0 ** (-1080.0 * rng.random(16) / max(n, 1))])
        xs.append(np.tile(x, 2))
        ns.append(np.full(64, n))
    for n in STRUCTURED_N:
        x = np.concatenate([EDGE_X, rng.random(60), 2.0 ** (-1080.0 * rng.random(60) / n)])
        xs.append(x)
        ns.append(np.full(128, n))
    xs, ns = np.concatenate(xs), np.concatenate(ns)
    assert xs.size % 64 == 0 and np.all(ns.reshape(-1, 64) == ns.reshape(-1, 64)[:, :1])
    uniq, inv = np.unique(np.stack([xs, ns.astype(np.float64)]), axis=1, return_inverse=True)
    want = X.exact_pow_array(uniq[0], uniq[1].astype(np.int64))[inv.ravel()]
    return xs, ns.astype(np.float64), want


def report_pow(what, got, want, sel=None):
    """Per band of the exact result: count, mismatches and the largest distance in ulps.  Zero
    mismatches where the result is >= 2**-969 or 0; below, within TINY_BAND_ULPS."""
    if sel is not None:
        got, want = got[sel], want[sel]
    d = X.ulps_apart(got, want)
    bands = [("normal >= 2^-969", want >= 2.0 ** -969, 0),
             ("[2^-1022, 2^-969)", (want >= 2.0 ** -1022) & (want < 2.0 ** -969), TINY_BAND_ULPS),
             ("subnormal", (want > 0) & (want < 2.0 ** -1022), TINY_BAND_ULPS),
             ("zero", want == 0, 0)]
    fails = []
    for name, m, allowed in bands:
        worst = int(d[m].max()) if m.any() else 0
        print(f"pow {what}: {name}: {int(m.sum())} operands, {int((d[m] != 0).sum())} differ, largest {worst} ulp")
        if worst > allowed:
            fails.append(f"{name}: largest {worst} ulp > {allowed} ({int((d[m] > allowed).sum())} operands)")
    assert not fails, f"pow {what}: " + "; ".join(fails)


def test_pow_uniform_exponent_per_wave(pow_set):
    """The scalar-controlled powering (one exponent per wave) against exact_pow; and the build with
    the general pow compiled in gives the same bits for these integral exponents."""
    xs, ns, want = pow_set
    got = ev(N.RT_EVAL_POW, xs, ns)
    report_pow("uniform n", got, want)
    assert_bits(ev(N.RT_EVAL_POW_GENERAL, xs, ns), got, "pow_libm<true> vs <false>, uniform n", (xs, ns))


def test_pow_exponent_per_lane(pow_set):
    """The same operands dealt so that every wave holds 64 different exponents (the per-lane loop)."""
    xs, ns, want = pow_set
    deal = np.arange(xs.size).reshape(-1, 64).T.ravel()
    assert np.all((ns[deal].reshape(-1, 64) != ns[deal].reshape(-1, 64)[:, :1]).any(axis=1))
    got = ev(N.RT_EVAL_POW, xs[deal], ns[deal])
    report_pow("per-lane n", got, want[deal])
    assert_bits(ev(N.RT_EVAL_POW_GENERAL, xs[deal], ns[deal]), got, "pow_libm<true> vs <false>, per-lane n",
                (xs[deal], ns[deal]))


def test_pow_inactive_lanes_carry_other_exponents(pow_set):
    """Waves whose inactive lanes (act = 0: the shading's lanes without a hit) hold another exponent —
    the first lane, the first half, a random half with the first lane, all but the last lane: the
    active lanes share theirs, so the scalar path runs, and they still get the right bits."""
    xs, ns, want = pow_set
    rng = np.random.default_rng(0x5EEDA)
    xs, ns = xs.copy().reshape(-1, 64), ns.copy().reshape(-1, 64)
    act = np.ones(xs.shape, dtype=np.uint8)
    lane = np.arange(64)
    for w in range(xs.shape[0]):
        off = [lane == 0, lane < 32, (rng.random(64) < 0.5) | (lane == 0), lane < 63][w % 4]
        act[w, off] = 0
        ns[w, off] = (ns[w, 0] + rng.integers(1, 1025, int(off.sum()))) % 1025  # never the wave's own
        xs[w, off] = rng.random(int(off.sum()))
    got = ev(N.RT_EVAL_POW, xs.ravel(), ns.ravel(), act=act.ravel())
    report_pow("inactive lanes", got, want, sel=act.ravel() != 0)


# ---- 1b. pow_libm<true> with the exponents mixed inside a wave --------------------------------
# A general-power scene's waves hold lanes that leave pow_libm<true> through the device's pow()
# (exponents that are no integer in 0..1024) beside lanes that take the binary powering, whose
# wave-uniform check (__ballot / readlane) then runs on the narrowed exec mask.
BIN_EXPONENTS = (0, 1, 4, 20, 1024)
LIB_EXPONENTS = (0.5, 2.5, 1025)
# HIP documents pow() in binary64 as within 1 ulp of the correctly rounded result
LIB_POW_ULPS = 1


@pytest.fixture(scope="module")
def mixed_wave_set():
    """(x, y, what) per wave of 64, x in [0, 1] (uniform, aimed at results over [2**-1080, 1] for each
    lane's exponent, and the edge x), the exponents dealt per lane:
      dealt        all eight exponents at random (32 waves)
      one_bin      exactly one lane on the binary powering (lane 0, 63, two random), every BIN exponent
      one_lib      exactly one lane through pow() (lane 0, 63, two random), every LIB exponent; the other
                   lanes share one BIN exponent (the scalar-controlled powering) or hold all five
      lib_lane0    lane 0 (readlane's fall-back) and a random third of the others through pow()
      lib_half     lanes 0..31 through pow(), lanes 32..63 one BIN exponent; and the other way round
      all_lib      no lane left for the binary powering"""
    rng = np.random.default_rng(0x5EED9B)
    lane = np.arange(64)
    waves = []

    def add(what, y):
        waves.append((what, np.asarray(y, dtype=np.float64)))

    for _ in range(32):
        add("dealt", rng.choice(BIN_EXPONENTS + LIB_EXPONENTS, 64))
    for n in BIN_EXPONENTS:
        for at in (0, 63, int(rng.integers(1, 63)), int(rng.integers(1, 63))):
            y = rng.choice(LIB_EXPONENTS, 64)
            y[at] = n
            add("one_bin", y)
    for e in LIB_EXPONENTS:
        for at in (0, 63, int(rng.integers(1, 63)), int(rng.integers(1, 63))):
            for n in BIN_EXPONENTS + (None,):
                y = rng.choice(BIN_EXPONENTS, 64) if n is None else np.full(64, n, dtype=np.float64)
                y = y.astype(np.float64)
                y[at] = e
                add("one_lib", y)
    for n in BIN_EXPONENTS + (None,):
        y = (rng.choice(BIN_EXPONENTS, 64) if n is None else np.full(64, n)).astype(np.float64)
        lib = (rng.random(64) < 1 / 3) | (lane == 0)
        y[lib] = rng.choice(LIB_EXPONENTS, int(lib.sum()))
        add("lib_lane0", y)
        for first in (True, False):
            y = np.full(64, BIN_EXPONENTS[1] if n is None else n, dtype=np.float64)
            y[(lane < 32) == first] = rng.choice(LIB_EXPONENTS, 32)
            add("lib_half", y)
    for _ in range(4):
        add("all_lib", rng.choice(LIB_EXPONENTS, 64))
    what = np.repeat([w for w, _ in waves], 64)
    ys = np.concatenate([y for _, y in waves])
    # x: a third uniform, a third aimed at the lane's own exponent, the edge values sprinkled over both
    xs = rng.random(ys.size)
    aimed = rng.random(ys.size) < 0.5
    xs[aimed] = 2.0 ** (-1080.0 * rng.random(int(aimed.sum())) / np.maximum(ys[aimed], 0.5))
    edge = rng.random(ys.size) < 0.05
    xs[edge] = rng.choice(EDGE_X[:6], int(edge.sum()))  # (x <= 1: the highlight's base is a cosine)
    is_bin = np.isin(ys, BIN_EXPONENTS)
    per_wave = is_bin.reshape(-1, 64).sum(axis=1)
    assert np.all(per_wave[what.reshape(-1, 64)[:, 0] == "one_bin"] == 1)
    assert np.all(per_wave[what.reshape(-1, 64)[:, 0] == "one_lib"] == 63)
    assert np.all(~is_bin.reshape(-1, 64)[what.reshape(-1, 64)[:, 0] == "lib_lane0", 0])
    assert np.all(per_wave[what.reshape(-1, 64)[:, 0] == "all_lib"] == 0)
    want = np.empty_like(xs)
    want[is_bin] = X.exact_pow_array(xs[is_bin], ys[is_bin].astype(np.int64))
    big = ys == 1025
    want[big] = X.exact_pow_array(xs[big], 1025)
    for e, k in ((0.5, 1), (2.5, 5)):
        m = ys == e
        want[m] = [X.exact_pow_half(float(x), k) for x in xs[m]]
    return xs, ys, what, is_bin, want


def test_pow_general_mixed_waves(mixed_wave_set):
    """RT_EVAL_POW_GENERAL on waves that mix the two kinds of exponent: the lanes on the binary
    powering equal the correctly rounded result bit for bit (under the rule for results below
    2**-969), in every arrangement; the lanes through pow() — 0.5 and 2.5 against the integer square
    root of the exact power, 1025 against the exact power — are within one unit in the last place."""
    xs, ys, what, is_bin, want = mixed_wave_set
    got = ev(N.RT_EVAL_POW_GENERAL, xs, ys)
    d = X.ulps_apart(got, want)
    fails = []
    for w in sorted(set(what.tolist())):
        m = (what == w) & ~is_bin
        worst = int(d[m].max()) if m.any() else 0
        i = int(np.argmax(np.where(m, d, -1)))
        print(f"pow mixed waves, {w}: {int(m.sum())} lanes through pow(), {int((d[m] != 0).sum())} not correctly "
              f"rounded, largest {worst} ulp (x = {float(xs[i]).hex()}, y = {ys[i]}, got {float(got[i]).hex()}, "
              f"want {float(want[i]).hex()})")
        if worst > LIB_POW_ULPS:
            fails.append(f"{w}: pow() {worst} ulp from the correctly rounded value at x = {float(xs[i]).hex()}, y = {ys[i]}")
    assert np.all(np.isfinite(got))
    for w in sorted(set(what.tolist())):
        m = (what == w) & is_bin
        if m.any():
            report_pow(f"mixed waves, {w}, binary powering", got, want, sel=m)
    assert not fails, "; ".join(fails)
    # the same operands with the lanes through pow() given an exponent of the binary powering: the
    # other lanes' bits do not depend on what their neighbours do
    alone = ev(N.RT_EVAL_POW_GENERAL, xs, np.where(is_bin, ys, 1.0))
    assert_bits(alone[is_bin], got[is_bin], "binary-powering lanes, with and without pow() lanes beside them",
                (xs[is_bin], ys[is_bin]))


# ---- 2. scenes with the exponents no other scene uses ---------------------------------------
# Pixels not bit-identical to the oracle: the oracle's pow is glibc's.  tests/test_exact_ref.py's
# glibc_pow_rates on 60,000 uniform x per exponent gives the fraction r of calls where it is not the
# correctly rounded value: n = 2, 3, 7, 1024: 0.00077, 0.00093, 0.00068, 0.00087; n = 5, 64, 255, 1023:
# 0.00085, 0.00110, 0.00069, 0.00083.  Bound = r (the set's largest) x the most pow calls a pixel
# makes (lights x depth) x 2 (the scene's operands are not uniform in x) x pixels:
#   default_powers: 0.00093 x (2 lights x 5) x 2 x (97 x 61 = 5917) = 110.06 -> 110
#   synthetic_mixed: 0.00110 x (4 lights x 5) x 2 x (96 x 80 = 7680) = 337.9 -> 337
@pytest.mark.parametrize("name,powers,w,h,bound", [("default_powers", (2, 3, 7, 1024), 97, 61, 110),
                                                   ("synthetic_mixed", (5, 64, 255, 1023), 96, 80, 337)])
def test_scenes_with_untested_integer_powers(oracle, name, powers, w, h, bound):
    """Specular powers that take the integer fast path but appear in no other scene (all squarings:
    1024; all multiplications: 1023, 255; odd small ones), on the fused engine (the default scene)
    and the wavefront engine (the mixed scene), depth 5: levels identical, max |delta| <= 1e-5."""
    scene = getattr(scenes, name)(powers=powers)
    img, lv = render(w, h, scene, 5, levels=True)
    ref, rlv = oracle.render(N.marshal(scene), w, h, 5, mode=oracle.MEMO, levels=True)
    _compare(img, lv, ref, rlv, f"{name}{powers}", bound)


# ---- 3. sqrt_x, div_n, normalize3 against the host's IEEE results ------------------------------
def _log_uniform(rng, count, elo, ehi):
    """Random 52-bit mantissas with exponents uniform in [elo, ehi)."""
    return np.ldexp(1.0 + rng.random(count), rng.integers(elo, ehi, count).astype(np.int32))


def _one_outlier_waves(rng, base, outliers):
    """For every outlier, four waves of in-range operands (rows of `base`) with that outlier in
    exactly one lane: the first, the last and two random lanes."""
    rows, k = [], 0
    for o in outliers:
        for lane in (0, 63, int(rng.integers(1, 63)), int(rng.integers(1, 63))):
            wave = base[64 * k:64 * (k + 1)].copy()
            wave[lane] = o
            rows.append(wave)
            k += 1
    return np.concatenate(rows)


def test_sqrt_bits():
    rng = np.random.default_rng(0x5EEDB)
    ints = rng.integers(-1024, 1025, (4096, 3)).astype(np.float64) * np.ldexp(1.0, -rng.integers(0, 16, (4096, 1)))
    m2 = (ints * ints).sum(axis=1)
    inr = np.concatenate([_log_uniform(rng, 8192, -767, 1000), m2[m2 > 0][:2048],
                          np.resize([2.0 ** -767, 2.0 ** 1000, np.nextafter(2.0 ** 1000, 0), 1.0, 4.0, 2.0], 64)])
    inr = inr[:inr.size // 64 * 64]
    assert np.all((inr >= 2.0 ** -767) & (inr <= 2.0 ** 1000))  # every wave takes the fast sequence
    assert_bits(ev(N.RT_EVAL_SQRT, inr), X.ref_sqrt(inr), "sqrt_x, waves in range", (inr,))
    # one lane outside [2^-767, 2^1000]: the whole wave takes the library's sqrt
    outl = [0.0, 2.0 ** -1074, 3.0 * 2.0 ** -1060, 2.0 ** -768, np.nextafter(2.0 ** -767, 0), 2.0 ** 1001,
            np.nextafter(2.0 ** 1000, np.inf), np.inf]
    mixed = _one_outlier_waves(rng, _log_uniform(rng, 64 * 4 * len(outl), -767, 1000), outl)
    assert np.all(((mixed < 2.0 ** -767) | (mixed > 2.0 ** 1000)).reshape(-1, 64).sum(axis=1) == 1)
    assert_bits(ev(N.RT_EVAL_SQRT, mixed), X.ref_sqrt(mixed), "sqrt_x, one lane out of range", (mixed,))


def test_div_bits():
    """div_n where its contract holds: |b| in [2^-400, 2^400], the quotient a normal number or 0."""
    rng = np.random.default_rng(0x5EEDC)
    sign = lambda k: np.where(rng.random(k) < 0.5, -1.0, 1.0)  # noqa: E731
    b = np.concatenate([_log_uniform(rng, 8192, -400, 400) * sign(8192),
                        rng.integers(1, 1 << 20, 4096).astype(np.float64),
                        np.resize([2.0 ** -400, 2.0 ** 400, -2.0 ** -400, -2.0 ** 400], 2048)])
    a = np.concatenate([np.ones(2048), _log_uniform(rng, 6144, -300, 300) * sign(6144),
                        rng.integers(0, 1 << 21, 4096).astype(np.float64),
                        np.resize([1.0, 0.0, 3.0, -1.0, 1.0 + 2.0 ** -52, 2.0 ** 300, 2.0 ** -300], 2048)])
    assert_bits(ev(N.RT_EVAL_DIV, a, b), X.ref_div(a, b), "div_n", (a, b))


def test_normalize3_bits():
    rng = np.random.default_rng(0x5EEDD)

    def vecs(count, elo, ehi):
        e = rng.integers(elo, ehi, (count, 1))
        v = (1.0 + rng.random((count, 3))) * np.where(rng.random((count, 3)) < 0.5, -1.0, 1.0)
        return np.ldexp(v * (rng.random((count, 3)) < 0.8), e.astype(np.int32))  # some components exactly 0

    ints = rng.integers(-1024, 1025, (4096, 3)).astype(np.float64) * np.ldexp(1.0, -rng.integers(0, 16, (4096, 1)))
    ends = np.array([[2.0 ** -200, 0, 0], [0, -2.0 ** 200, 0], [0, 0, 2.0 ** -200], [2.0 ** 200, 0, 0],
                     [3.0, 0.0, 4.0], [1.0, 1.0, 1.0], [-1.0, 2.0, -2.0], [2.0 ** 199, 2.0 ** 199, 2.0 ** 199]])
    inr = np.concatenate([vecs(8192, -198, 198), ints, np.resize(ends, (64, 3))])
    m2 = (inr * inr).sum(axis=1)
    inr = inr[(m2 >= 2.0 ** -400) & (m2 <= 2.0 ** 400)]
    inr = inr[:inr.shape[0] // 64 * 64]
    assert inr.shape[0] >= 8192
    assert_bits(ev(N.RT_EVAL_NORMALIZE3, inr), X.ref_normalize3(inr), "normalize3, waves in range", (inr,))
    # one lane with m2 = 0, below 2^-400 or above 2^400 (to underflow and overflow of m2): the whole
    # wave takes the library's sqrt and division, and the zero vector gives (0, 0, 0)
    outl = [[0.0, 0.0, 0.0], [2.0 ** -201, 0.0, 0.0], [2.0 ** -210, -2.0 ** -205, 2.0 ** -220], [1e-170, 1e-180, 0.0],
            [2.0 ** -1074, 0.0, 0.0], [2.0 ** 201, 0.0, 0.0], [2.0 ** 210, 2.0 ** 205, -2.0 ** 220], [1e200, -1e200, 1e10]]
    base = vecs(64 * 4 * len(outl) + 512, -198, 198)
    bm2 = (base * base).sum(axis=1)
    base = base[(bm2 >= 2.0 ** -400) & (bm2 <= 2.0 ** 400)]
    mixed = _one_outlier_waves(rng, base, [np.array(o) for o in outl])
    with np.errstate(over="ignore"):
        mm2 = (mixed * mixed).sum(axis=1)
    assert np.all((~((mm2 >= 2.0 ** -400) & (mm2 <= 2.0 ** 400))).reshape(-1, 64).sum(axis=1) == 1)
    assert_bits(ev(N.RT_EVAL_NORMALIZE3, mixed), X.ref_normalize3(mixed), "normalize3, one lane out of range",
                (mixed,))


# ---- 4. div_dim, idiv_dim against exact division -----------------------------------------------
DIMS = sorted({1 << k for k in range(21)} | {(1 << k) + 1 for k in range(1, 20)} | {(1 << k) - 1 for k in range(1, 21)}
              | {3, 61, 97, 480, 640, 1080, 1920, 1048575})


def test_div_dim_bits():
    """div_dim(a, n) == a / n.  Its call sites (primary_dir): a = x or x + u with an integer
    0 <= x < n <= 2^20 and u = k * 2^-24, k < 2^24 — exact binary64 values with at most 44 bits; and
    the documented domain, integers below 2^44."""
    rng = np.random.default_rng(0x5EEDE)
    for n in DIMS:
        x = np.concatenate([[0, n - 1, n // 2], rng.integers(0, n, 381)]).astype(np.float64)
        u = np.concatenate([[0, 1, (1 << 24) - 1], rng.integers(0, 1 << 24, 381)]).astype(np.float64) * 2.0 ** -24
        a = np.concatenate([x, x + u, rng.integers(0, 1 << 44, 253).astype(np.float64), [0.0, 2.0 ** 44 - 1, 1.0]])
        assert a.size == 1024
        assert_bits(ev(N.RT_EVAL_DIV_DIM, a, dim=n), X.ref_div(a, float(n)), f"div_dim n={n}", (a,))


def test_idiv_dim_exact():
    """idiv_dim(a, n) == a // n for 0 <= a < 2^31 (rec0_to_rec: a pixel index by the width, a slab
    row by the row block), with the multiples of n and their neighbours up to 2^31 - 1."""
    rng = np.random.default_rng(0x5EEDF)
    top = (1 << 31) - 1
    for n in DIMS:
        kmax = top // n
        k = np.unique(np.concatenate([[0, 1, 2, kmax - 1, kmax], rng.integers(0, kmax + 1, 200)]))
        k = k[(k >= 0) & (k <= kmax)]
        near = np.concatenate([k * n - 1, k * n, k * n + 1])
        a = np.concatenate([near[(near >= 0) & (near <= top)], [0, top], rng.integers(0, 1 << 31, 400)])
        got = ev(N.RT_EVAL_IDIV_DIM, a.astype(np.float64), dim=n)
        want = X.ref_floordiv(a, n)
        bad = np.nonzero(got != want.astype(np.float64))[0]
        assert bad.size == 0, f"idiv_dim n={n}: a={a[bad[:5]]} got {got[bad[:5]]} want {want[bad[:5]]}"

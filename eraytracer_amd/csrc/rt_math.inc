// rt_math.inc — the binary64 primitives, included inside rt_render.hip's anonymous namespace:
// D3 and the reference's vector operations, the correctly rounded sqrt / division fast paths
// (sqrt_n, div_n, div_dim, idiv_dim, sqrt_x, normalize3), the integer powering (pow_bin, pow_libm)
// and the primitive tests (sph_t, tri_t, pl_t, sph_t_wave, nearer).
// Expects: <hip/hip_runtime.h>; nothing else of this translation unit.

struct D3 {
    double x, y, z;
};

__device__ __forceinline__ double dot3(const D3 &a, const D3 &b) { // vector_dot_product/2 (:546-547)
    return a.x * b.x + a.y * b.y + a.z * b.z;
}

// ---- correctly rounded sqrt and division, bit for bit the compiler's, minus range handling --
// The device sqrt(double) is v_rsq_f64 refined by one Goldschmidt and two Newton steps, wrapped
// in a scaling for inputs below 2^-767 and fix-ups for 0 and inf; 1.0/b is v_rcp_f64 refined
// twice, one correction step, wrapped in v_div_scale / v_div_fmas / v_div_fixup, which leave
// operands and results unchanged for normal-range values.  The *_n forms are those refinement
// sequences alone (operand for operand, so the same bits) and are used only where every lane's
// operand is inside the range where the wrappers are the identity; *_x check that for the wave
// (one compare and a ballot) and otherwise take the full device sequence.  About 40 % fewer
// VALU instructions per normalize (S64 4096^2 d5: 25.3 -> 26.4 Gpx/s).  Not used in the beam
// culling: there the extra wave-uniform branches cost more than they saved (measured).
constexpr double SQRT_N_LO = 0x1p-767, SQRT_N_HI = 0x1p1000;
constexpr double RCP_N_LO = 0x1p-400, RCP_N_HI = 0x1p400;

__device__ __forceinline__ double sqrt_n(double x) {
    const double s = __builtin_amdgcn_rsq(x);
    double g = x * s;
    double h = s * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}

// a / b for |b| in [RCP_N_LO, RCP_N_HI] and |a| small enough that a/b is a normal number or 0
__device__ __forceinline__ double div_n(double a, double b) {
    double y = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    const double q = a * y;
    const double r = __builtin_fma(-b, q, a);
    return __builtin_fma(r, y, q);
}

// a / n for a frame dimension n (W, H; 1 <= n <= 2^20) and 0 <= a < 2^44 exactly representable:
// for a power of two the quotient is exact, so the correctly rounded division is the exponent
// shift (one v_ldexp_f64 instead of v_rcp_f64 and seven fma / mul) — the same bits.  n (uniform)
// is made opaque where it is used: otherwise the compiler hoists (double) n and its reciprocal out
// of the kernels' record loops into VGPRs that stay live (and spilled) across everything.
// A wave-uniform value made opaque where it is used: a test on it (and what the compiler derives from
// it) is evaluated there, in a few SALU instructions, instead of being hoisted out of the record loops
// as a 64-bit condition mask held in SGPRs — which spilled to VGPR lanes (v_writelane / v_readlane).
template <typename T>
__device__ __forceinline__ T opq(T v) {
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ double div_dim(double a, int n) {
    n = opq(n);
    if ((n & (n - 1)) == 0) return __builtin_amdgcn_ldexp(a, -__builtin_ctz((unsigned)n)); // (wave-uniform)
    return div_n(a, (double)n);
}
// floor(a / n) for 0 <= a < 2^31, 1 <= n <= 2^20: a shift for a power of two; otherwise the
// correctly rounded binary64 quotient, which truncates to the exact integer quotient
__device__ __forceinline__ int idiv_dim(int a, int n) {
    n = opq(n);
    if ((n & (n - 1)) == 0) return a >> __builtin_ctz((unsigned)n); // (wave-uniform)
    return (int)div_n((double)a, (double)n);
}
// The lane's index in its wave, opaque to the optimiser: lane masks derived from it are recomputed
// where they are used (two instructions) instead of being hoisted out of the record loops and kept
// live — or spilled — across the shading.
__device__ __forceinline__ int lane_id() {
    int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(l));
    return l;
}

// FAST: the caller guarantees x is in range (a sphere test's discriminant, >= 0.001 or 1.0 by
// then, in a spheres-only scene within CULL_EXTENT: every ray is a unit vector — primary rays and
// shadow rays are normalised, reflections off spheres keep the length — so disc <= ~1e10, far
// below 2^1000), and the check is skipped.
template <bool FAST = false>
__device__ __forceinline__ double sqrt_x(double x) { // == sqrt(x)
    // (the fast sequence inside the wave-uniform branch: measured 3-6 % faster per frame than
    // computing it unconditionally and redoing out-of-range waves)
    if (FAST || __ballot(!(x >= SQRT_N_LO && x <= SQRT_N_HI)) == 0) return sqrt_n(x);
    return sqrt(x);
}

// fast (wave-uniform): the host proved m2 inside the range (SceneHdr::norm_ok / prim_ok)
__device__ __forceinline__ D3 normalize3(const D3 &v, bool fast = false) { // vector_normalize/1 (:554-560)
    const double m2 = v.x * v.x + v.y * v.y + v.z * v.z;
    if (fast || __ballot(!(m2 >= RCP_N_LO && m2 <= RCP_N_HI)) == 0) { // mag and 1/mag in range, mag != 0
        const double s = div_n(1.0, sqrt_n(m2));
        return D3{v.x * s, v.y * s, v.z * s};
    }
    double mag = sqrt(m2);
    double s = 1.0 / mag;
    D3 r = {v.x * s, v.y * s, v.z * s};
    if (mag == 0) r = D3{0.0, 0.0, 0.0};
    return r;
}

__device__ __forceinline__ D3 bounce3(const D3 &v, const D3 &n) { // vector_bounce_off_plane/2 (:568-573)
    double k = 2 * (n.x * -v.x + n.y * -v.y + n.z * -v.z);
    return D3{n.x * k + v.x, n.y * k + v.y, n.z * k + v.z};
}

__device__ __forceinline__ double max0(double x) { return x > 0 ? x : 0.0; } // lists:max([0, X])

// math:pow/2 (:289) is the host libm's pow, which is correctly rounded for all but
// vanishingly rare arguments.  For the small non-negative integer exponents scenes use
// (specular_power 1, 4, 20; any integer 0..1024 takes this path) the kernel evaluates x^n by
// binary powering in double-double arithmetic, then one rounding — cheaper than, and closer to
// libm than, the device's general pow.  The pairs hi + lo are kept unnormalised, so a step is
// one product and its fma error terms; the fma calls are error-free product transformations, not
// contractions.  lo is the product's exact low part plus the cross terms, and a squaring doubles
// lo / hi: after k squarings |lo| is up to ~2^k ulp(hi) (2^-43 hi for n = 1024, not a fixed
// ~2 ulp), and the dropped lo^2 and lo lo' terms leave a relative error of ~2^-100 for the
// exponents scenes use (n <= 20) growing to ~2^-86 at n = 1024.  That is far inside half an ulp,
// so the result is the correctly rounded one unless x^n lies within that distance of a rounding
// boundary (about one operand in 2^33 at n = 1024): tests/test_gpu_math_exact.py compares it bit for
// bit with exact integer arithmetic for every n in 0..1024 (and tests/test_exact_ref.py restates
// it on the CPU).  That holds for results >= 2^-969 and for results that round to 0.  Below
// 2^-969 a pair's low part is itself subnormal, so the fma error terms are rounded, and in the
// subnormal band hi + lo is a second rounding: there the result is within one unit in the last
// place (2^-1074 in the subnormal band) of the correctly rounded value, and differs from it for
// ~2 % of the operands in [2^-1022, 2^-969) and ~5 % of the subnormal ones; the oracle's glibc
// pow is the correct one there.  (At most 2^-1022 in a highlight term: invisible next to the 1e-5
// bar.  A repair — redo such lanes from x scaled into [0.75, 1.5), round once at the result's
// quantum — gave the exact bits but cost config 3 2 % by its mere presence in the shading
// kernels, registers and SGPR spills: profiles/pow_tiny_ab.txt.)
__device__ __forceinline__ void dd_sqr(double &h, double &l) {
    const double p = h * h;
    const double e = __builtin_fma(h + h, l, __builtin_fma(h, h, -p));
    h = p;
    l = e;
}
__device__ __forceinline__ void dd_mul(double &ah, double &al, double bh, double bl) {
    const double p = ah * bh;
    const double e = __builtin_fma(al, bh, __builtin_fma(ah, bl, __builtin_fma(ah, bh, -p)));
    ah = p;
    al = e;
}
// GENPOW: the scene has a specular power outside {0, 1, ..., 1024} (SceneHdr::int_pow = 0, decided on
// the host by shading_tables in rt_scene.cpp), so the general device pow is compiled in; otherwise its large
// register footprint is kept out of the kernel.
// x^n, n >= 1, by binary powering (the operations depend on n alone).  BR (n wave-uniform): the
// multiplications sit under a branch the empty asm keeps one (if-converted, each ran for every step
// behind four v_cndmask per double-double); for a per-lane n the selects measured faster than exec-
// masked branches (config 3's dominant kernel +1.2 %, profiles/r06u_ab_pow.txt).
template <bool BR, typename U>
__device__ __forceinline__ double pow_bin(double x, U n) {
    double bh = x, bl = 0.0;
    while (!(n & 1u)) { // x^(2^k) for the lowest set bit: the result starts there
        dd_sqr(bh, bl);
        n >>= 1;
    }
    double rh = bh, rl = bl;
    while (n >>= 1) {
        dd_sqr(bh, bl);
        if (n & 1u) {
            if (BR) asm volatile("");
            dd_mul(rh, rl, bh, bl);
        }
    }
    return rh + rl;
}
// act: the lanes whose result is used.  A wave's records mostly lie on one object: when all of its
// active lanes share the exponent, the powering runs under scalar control (the exponent read from
// one lane), with no per-lane loop masks; otherwise each lane loops on its own.  The same operations
// either way, so the same bits.
template <bool GENPOW>
__device__ __forceinline__ double pow_libm(double x, double y, bool act = true) {
    if (GENPOW && !(y >= 0.0 && y <= 1024.0 && y == __builtin_floor(y))) return pow(x, y);
    const unsigned n = (unsigned)y;
    const unsigned long long am = __ballot(act);
    const unsigned n0 = (unsigned)__builtin_amdgcn_readlane((int)n, am ? __builtin_ctzll(am) : 0);
    if (__ballot(act && n != n0) == 0) return n0 == 0 ? 1.0 : pow_bin<true>(x, n0); // (wave-uniform)
    return n == 0 ? 1.0 : pow_bin<false>(x, n);
}

// ---- primitive tests: return true and t on a valid hit --------------------------------------
// ray_sphere_intersect/2 (:364-397), from B and C (A4 = 4*A hoisted per ray)
template <bool FAST = false>
__device__ __forceinline__ bool sph_t(double B, double C, double A4, double &t) {
    double disc = B * B - A4 * C;
    if (!(disc >= 0.001)) return false;
    double sq = sqrt_x<FAST>(disc);
    // T0 = (-B + sq)/2, T1 = (-B - sq)/2 (:379-383) with sq > 0: T1 <= T0 after rounding too (rounding
    // is monotonic), so lists:min([T0, T1]) is T1 (bit for bit where the two are equal) and both are
    // >= 0 iff T1 is (NaN and infinite B or disc fail either way) — T0 is never needed
    t = (-B - sq) / 2;
    return t >= 0;
}

// ray_triangle_intersect/2 (:402-455), with T = O - v1 and Q = T x Edge1 given
__device__ __forceinline__ bool tri_t(const D3 &d, const D3 &e1, const D3 &e2, const D3 &T, const D3 &Q,
                                      double &t) {
    D3 P = {d.y * e2.z - d.z * e2.y, d.z * e2.x - d.x * e2.z, d.x * e2.y - d.y * e2.x};
    double det = dot3(e1, P);
    if (det < 0.000001) return false;
    double U = dot3(T, P);
    if ((U < 0) || (U > det)) return false;
    double V = dot3(d, Q);
    if ((V < 0) || (U + V > det)) return false;
    t = dot3(e2, Q) / det;
    return true;
}

// ray_plane_intersect/2 (:461-480), with V0 = -(N.O + Distance) given
__device__ __forceinline__ bool pl_t(const D3 &n, const D3 &d, double V0, double &t) {
    double Vd = dot3(n, d);
    if (!(Vd < 0)) return false;
    t = V0 / Vd;
    if (t < 0.001) return false;
    return true;
}

// The same decision as sph_t without divergent branches: the root computation runs for the
// whole wave unless no lane can hit (a wave-uniform test), and the outcome is a mask.
template <bool FAST = false>
__device__ __forceinline__ bool sph_t_wave(double B, double C, double A4, double &t) {
    const double disc = B * B - A4 * C;
    const bool ok = disc >= 0.001;
    t = 0.0;
    if (__ballot(ok) == 0) return false;
    // FAST: the failing lanes' roots (NaN for disc < 0) are dropped by `ok` below; only the range-checked
    // form needs them in range, lest they send the wave down the full sqrt
    const double sq = sqrt_x<FAST>(FAST || ok ? disc : 1.0);
    t = (-B - sq) / 2; // the nearer root (sph_t)
    return ok & (t >= 0);
}

// (without the short circuit — no divergent branch per candidate — measured config 3 +0.9 %, config 5
// -0.7 %: profiles/r05af_ab_nearer_no_short_circuit.txt)
__device__ __forceinline__ bool nearer(double t, int id, double bt, int bid) {
    return t < bt || (t == bt && id < bid); // first in list order among equal distances (:319)
}

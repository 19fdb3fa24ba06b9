// rt_selftest.inc — the arithmetic self-test kernels behind rt_selftest_math and rt_eval_math,
// included inside rt_render.hip's anonymous namespace.
// Expects: rt_math.inc, the wave reductions and lane_f32 of rt_cull.inc, and splitmix64 (rt_primary.inc).

// rt_selftest_math: sqrt_n / div_n against the device library's sqrt and division, bit for bit,
// on operands spread log-uniformly over the ranges where the kernels use them; pow_libm's wave-
// uniform path against the per-lane powering; the binary32 wave reductions against a lane loop.
__global__ __launch_bounds__(256) void k_selftest_math(unsigned long long n, unsigned long long seed,
                                                       unsigned long long *__restrict__ bad) {
    unsigned long long local = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long r = splitmix64(seed ^ i), r2 = splitmix64(seed ^ ~i);
        // sqrt over [2^-767, 2^1000]: random exponent, random 52-bit mantissa
        const long long e = 1023 - 767 + (long long)((r >> 52) % (767 + 1000));
        const double x = __longlong_as_double((long long)((unsigned long long)e << 52 | (r & 0xFFFFFFFFFFFFFull)));
        if (__double_as_longlong(sqrt_n(x)) != __double_as_longlong(sqrt(x))) ++local;
        // structured operands (scenes are written with small integers and short fractions): the
        // squared length of a vector of integers in [-2^10, 2^10] scaled by 2^-k
        {
            const double sx = (double)((long long)(r & 0x7FF) - 1024), sy = (double)((long long)((r >> 11) & 0x7FF) - 1024),
                         sz = (double)((long long)((r >> 22) & 0x7FF) - 1024);
            const double sc = __builtin_amdgcn_ldexp(1.0, -(int)((r >> 33) & 15));
            const D3 w = {sx * sc, sy * sc, sz * sc};
            const D3 uw = normalize3(w);
            const double mw = sqrt(w.x * w.x + w.y * w.y + w.z * w.z), sw = 1.0 / mw;
            if (mw != 0 && (__double_as_longlong(uw.x) != __double_as_longlong(w.x * sw) ||
                            __double_as_longlong(uw.y) != __double_as_longlong(w.y * sw) ||
                            __double_as_longlong(uw.z) != __double_as_longlong(w.z * sw)))
                ++local;
        }
        // 1/b and a/b: b over [2^-400, 2^400], a an integer below 2^21 (the primary-ray divisions)
        const long long eb = 1023 - 400 + (long long)((r2 >> 52) % 800);
        const double b = __longlong_as_double((long long)((unsigned long long)eb << 52 | (r2 & 0xFFFFFFFFFFFFFull)));
        if (__double_as_longlong(div_n(1.0, b)) != __double_as_longlong(1.0 / b)) ++local;
        const double a = (double)(r >> 43), w = (double)((r2 >> 44) + 1);
        if (__double_as_longlong(div_n(a, w)) != __double_as_longlong(a / w)) ++local;
        // normalize3 on random vectors (both paths)
        const D3 v = {x * (r & 1 ? 1 : -1) * 0x1p-600, b * 1e-3, a - 1e6};
        const D3 u = normalize3(v);
        const double m = sqrt(v.x * v.x + v.y * v.y + v.z * v.z), sc = 1.0 / m;
        if (m != 0 && (__double_as_longlong(u.x) != __double_as_longlong(v.x * sc) ||
                       __double_as_longlong(u.y) != __double_as_longlong(v.y * sc) ||
                       __double_as_longlong(u.z) != __double_as_longlong(v.z * sc)))
            ++local;
        // pow_libm's scalar-controlled powering (a wave-uniform exponent: one per 64 consecutive i,
        // every other group) against the per-lane powering, bit for bit; x over [0, 1 + 2^-20)
        {
            const double px = (double)(r2 & 0xFFFFFFFFFFFull) * 0x1p-44 * (1.0 + 0x1p-20);
            const unsigned pu = (unsigned)(splitmix64(seed ^ (i >> 6)) % 1025u), pl = (unsigned)((r2 >> 44) % 1025u);
            const unsigned pn = ((i >> 6) & 1) ? pu : pl;
            const double want = pn == 0 ? 1.0 : pow_bin<false>(px, pn);
            if (__double_as_longlong(pow_libm<false>(px, (double)pn)) != __double_as_longlong(want)) ++local;
        }
        // the binary32 wave reductions (whole waves only): the maximum of values >= +0 exactly, the
        // minimum exactly when no value is negative and negative when one is
        if (__ballot(true) == ~0ull) {
            const float f0 = (float)((double)(r & 0xFFFFFF) * 0x1p-20);
            const float fv = (r >> 40) % 97 == 0 ? -1.0f - f0 : f0; // (no -0.0: its bits order below +0.0's)
            const float fa = __builtin_fabsf(fv);
            float tmin = 3.0e38f, tmax = 0.0f;
            bool neg = false;
            for (int l = 0; l < 64; ++l) { // (wave-uniform)
                const float a = lane_f32(fv, l), b = lane_f32(fa, l);
                tmin = a < tmin ? a : tmin;
                tmax = b > tmax ? b : tmax;
                neg = neg || a < 0.0f;
            }
            const float gmin = wave_min32(fv), gmax = wave_max32(fa);
            if (__float_as_int(gmax) != __float_as_int(tmax) || (neg ? !(gmin < 0.0f) : __float_as_int(gmin) != __float_as_int(tmin)))
                ++local;
        }
    }
    if (local) atomicAdd(bad, local);
}

// rt_eval_math: one operand per work-item in array order (elements 64k .. 64k+63 are one wave, so
// the caller's operand order decides what is wave-uniform), through the functions the render
// kernels call.  dim reaches div_dim / idiv_dim as a kernel argument (wave-uniform, as W, H and
// the row block are at their call sites).
template <int OP>
__global__ __launch_bounds__(256) void k_eval_math(unsigned long long n, const double *__restrict__ a,
                                                   const double *__restrict__ b,
                                                   const unsigned char *__restrict__ act, int dim,
                                                   double *__restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (OP == RT_EVAL_NORMALIZE3) {
        const D3 u = normalize3(D3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}, false);
        out[3 * i] = u.x;
        out[3 * i + 1] = u.y;
        out[3 * i + 2] = u.z;
        return;
    }
    const double x = a[i];
    double r;
    if (OP == RT_EVAL_POW) r = pow_libm<false>(x, b[i], act ? act[i] != 0 : true);
    else if (OP == RT_EVAL_POW_GENERAL) r = pow_libm<true>(x, b[i]);
    else if (OP == RT_EVAL_SQRT) r = sqrt_x<false>(x);
    else if (OP == RT_EVAL_DIV) r = div_n(x, b[i]);
    else if (OP == RT_EVAL_DIV_DIM) r = div_dim(x, dim);
    else r = (double)idiv_dim((int)x, dim);
    out[i] = r;
}

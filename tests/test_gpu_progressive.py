"""Progressive supersampling on the GPU (RT_PROGRESSIVE in include/rt_mi355x.h): rt_launch_samples
folds a range of a frame's samples into a caller-owned binary64 sum, rt_resolve turns a sum into a
frame of any RT_OUT_* format.

The yardstick of G1 is rt_launch_window with the same arguments on a fresh context: whatever the
partition of the samples, the resolved sum must equal its slab in every byte, levels included.  Every
sum and levels buffer is pre-filled with a sentinel and followed by 16 guard rows: the slab rows past
the image and the guard rows must keep it.  rt_resolve is checked against numpy (binary64 division,
astype(float32), the integer rule of tests/test_gpu_int_frames.ref_quant), and the partial sums
against the C oracle through a restatement of the sample positions made here from the header.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import scenes
from eraytracer_amd.dist import shard_global_rows
from tests.test_gpu_int_frames import adversarial, ref_quant
from tests.test_gpu_primary_tiles import LV_SENTINEL, SENTINEL, Ctx, bits, same
from tests.test_gpu_window import launch as launch_window

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, DEPTH, GUARD = 200, 150, 5, 16
WIN = (37, 21, 83, 59)
SEED = 0x5EED0004
FMT = {"f64": N.RT_OUT_F64, "f32": N.RT_OUT_F32, "u8": N.RT_OUT_U8, "u16": N.RT_OUT_U16}
NP_DT = {"f64": np.float64, "f32": np.float32, "u8": np.uint8, "u16": np.uint16}
PARTITIONS = [[(0, 4)], [(0, 1), (1, 4)], [(0, 3), (3, 4)], [(0, 2), (2, 4)], [(0, 1), (1, 2), (2, 3), (3, 4)]]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def resolve_dev(d_ptr, n, samples, prec, maxv, out_ptr, cnt_ptr=None):
    N.check(N.lib().rt_resolve(d_ptr, n, samples, FMT[prec], maxv, out_ptr, cnt_ptr, stream()), "rt_resolve")


class Sum:
    """A sentinel-filled sum slab and levels buffer, GUARD rows after each, for one frame geometry."""

    def __init__(self, c, iw, ih, win, d=DEPTH, *, spp, seed=SEED, rb=16, shard=0, nshards=1, levels=True):
        import torch
        self.c, self.args = c, (iw, ih, d, *win, rb, shard, nshards, spp, seed)
        self.w, self.h, self.spp = win[2], win[3], spp
        self.rows = c.L.rt_shard_rows(self.h, rb, nshards)
        self.valid = int((shard_global_rows(self.h, rb, nshards, shard) >= 0).sum())  # a prefix of the slab
        self.sum = torch.full((self.rows + GUARD, self.w, 3), SENTINEL, dtype=torch.float64, device="cuda")
        self.lv = torch.full((self.rows + GUARD, self.w), LV_SENTINEL, dtype=torch.uint8, device="cuda")
        self.levels = levels

    def refill(self):
        self.sum.fill_(SENTINEL)
        self.lv.fill_(LV_SENTINEL)

    def add(self, begin, end):
        rc = self.c.L.rt_launch_samples(self.c.p, *self.args, begin, end, self.sum.data_ptr(),
                                        self.lv.data_ptr() if self.levels else None, stream())
        assert rc == N.RT_OK, (rc, begin, end)
        return self

    def host(self):
        """(sum, levels) on the host, after checking that nothing outside the image's rows was written."""
        import torch
        torch.cuda.synchronize()
        s, lv = self.sum.cpu().numpy(), self.lv.cpu().numpy()
        assert np.all(s[self.valid:] == SENTINEL), "sum rows past the image (or guard rows) written"
        assert np.all(lv[self.valid:] == LV_SENTINEL), "level rows past the image (or guard rows) written"
        assert not np.any(s[:self.valid] == SENTINEL), "a pixel of the sum was never stored"
        if not self.levels:
            assert np.all(lv == LV_SENTINEL)
        return s, lv

    def resolve(self, prec, samples=None, maxv=255):
        """The frame of the sum's rows inside the image, in a sentinel-filled buffer of the sum's shape
        (what rt_launch_window leaves of such a buffer), and the clamped count."""
        import torch
        dt = {"f64": torch.float64, "f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}[prec]
        fill = SENTINEL if prec in ("f64", "f32") else LV_SENTINEL
        out = torch.full(tuple(self.sum.shape), fill, dtype=dt, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        resolve_dev(self.sum.data_ptr(), self.valid * self.w * 3, samples or self.spp, prec, maxv, out.data_ptr(),
                    cnt.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy(), int(cnt.item())


@functools.lru_cache(maxsize=None)
def one_shot(name, iw, ih, win, d, prec, spp, seed, side, levels, cull=True, rb=16, shard=0, nshards=1):
    """rt_launch_window with RT_ORDER_EXACT on a fresh context: (slab with GUARD rows, levels), read-only."""
    with Ctx(scenes.named(name), cull=cull, side=side) as c:
        img, lv = launch_window(c, iw, ih, win, d, prec=prec, rb=rb, shard=shard, nshards=nshards, spp=spp, seed=seed,
                                levels=levels)
    img.setflags(write=False)
    lv.setflags(write=False)
    return img, lv


def check_g1(name, iw, ih, win, d, *, side, levels, cull=True, partitions=PARTITIONS, spp=4, seed=SEED, **geom):
    """Every partition on one context (a call with sample_begin = 0 restarts the frame), resolved to
    f64 and f32, against the one-shot slab of a fresh context: every byte, the levels too."""
    with Ctx(scenes.named(name), cull=cull, side=side) as c:
        s = Sum(c, iw, ih, win, d, spp=spp, seed=seed, levels=levels, **geom)
        for part in partitions:
            s.refill()
            for b, e in part:
                s.add(b, e)
            _, lv = s.host()
            for prec in ("f64", "f32"):
                ref, rlv = one_shot(name, iw, ih, win, d, prec, spp, seed, side, levels, cull, **geom)
                got, _ = s.resolve(prec)
                assert same(got, ref), (name, part, prec, int((bits(got) != bits(ref)).any(axis=-1).sum()), "pixels differ")
                assert np.array_equal(lv, rlv), (name, part, int((lv != rlv).sum()))
    return s


# ---- 1. G1: any partition gives the frame -----------------------------------------------------
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("levels", [True, False])
@pytest.mark.parametrize("side", [None, 0, 1])
def test_any_partition_gives_the_frame(side, levels, cull):
    """S64 at 200x150 depth 5, four samples: side streams default / off / on and levels on / off take
    both ways of summing (the pass folds its sample itself; a sample slab and k_accum)."""
    s = check_g1("s64", W, H, (0, 0, W, H), DEPTH, side=side, levels=levels, cull=cull)
    assert s.rows == 160 and s.valid == 150  # ten padding rows and the guard rows kept their sentinel
    ref, lv = one_shot("s64", W, H, (0, 0, W, H), DEPTH, "f64", 4, SEED, side, levels, cull)
    one = one_shot("s64", W, H, (0, 0, W, H), DEPTH, "f64", 1, 0, side, levels, cull)[0]
    assert not same(ref, one), "the supersampled frame is the one-sample frame"
    if levels:
        assert set(lv[:H].ravel().tolist()) == {0, 1, 2, 3, 4, 5}  # every reflection level is populated


# ---- 2. G1 on the other shapes ------------------------------------------------------------------
TWO = [[(0, 1), (1, 4)], [(0, 3), (3, 4)]]
# (side, levels): the sample-slab path, and the path where every pass folds its own sample
PATHS = [(None, True), (0, False)]


@pytest.mark.parametrize("side,levels", PATHS)
def test_window(side, levels):
    check_g1("s64", W, H, WIN, DEPTH, side=side, levels=levels, partitions=TWO)


@pytest.mark.parametrize("side,levels", PATHS)
def test_shard_with_padding_rows(side, levels):
    """Shard 1 of 3, row_block 16: the slab has 64 rows of which 48 lie in the image (rows 16-31,
    64-79, 112-127), and those 16 rows of padding must not be written in d_sum."""
    s = check_g1("s64", W, H, (0, 0, W, H), DEPTH, side=side, levels=levels, partitions=TWO, rb=16, shard=1, nshards=3)
    assert (s.rows, s.valid) == (64, 48)
    s = check_g1("s64", W, H, (0, 0, W, H), DEPTH, side=side, levels=levels, partitions=TWO[:1], rb=16, shard=2, nshards=3)
    assert (s.rows, s.valid) == (64, 48)


@pytest.mark.parametrize("side,levels", PATHS + [(None, False)])
@pytest.mark.parametrize("name,w,h,d", [("s64l0", 200, 150, 5), ("s64l40", 200, 150, 5), ("mixed", 96, 64, 5),
                                        ("s256", 64, 48, 8)])
def test_other_scenes(name, w, h, d, side, levels):
    """No lights (no reflections: single write even with side streams), more than 32 lights (the walks
    re-test shadows), triangles / planes / the general pow, and the BVH levels of S256 at depth 8."""
    check_g1(name, w, h, (0, 0, w, h), d, side=side, levels=levels, partitions=TWO)


@pytest.mark.parametrize("side,levels", PATHS)
@pytest.mark.parametrize("d", [0, 1])
def test_depth_0_and_1(d, side, levels):
    check_g1("s64", W, H, (0, 0, W, H), d, side=side, levels=levels, partitions=TWO)
    if d == 0:  # all background: sample 0 stores +0.0 over the sentinel, sign bit included
        with Ctx(scenes.s64(), side=side) as c:
            s = Sum(c, W, H, (0, 0, W, H), 0, spp=4, levels=levels).add(0, 1)
            assert np.all(bits(s.host()[0][:H]) == 0)
            assert np.all(bits(s.add(1, 4).host()[0][:H]) == 0)


# ---- 3. G2: the sum does not depend on the partition ---------------------------------------------
@functools.lru_cache(maxsize=None)
def partial_sums(side, levels):
    """S64, spp 5: the sums after [0,3) (one call), [0,3) (two calls), [0,5), and a restart's [0,3)."""
    with Ctx(scenes.s64(), side=side) as c:
        s = Sum(c, W, H, (0, 0, W, H), DEPTH, spp=5, levels=levels)
        a, lv = s.add(0, 3).host()
        s.refill()
        b = s.add(0, 1).add(1, 3).host()[0]
        full = s.add(3, 5).host()[0]
        r = s.add(0, 3).host()[0]  # sample_begin = 0 into a used sum: the frame restarts
    return a, b, full, r, lv


@pytest.mark.parametrize("side,levels", PATHS)
def test_sum_does_not_depend_on_the_partition(side, levels):
    a, b, full, r, _ = partial_sums(side, levels)
    assert same(a, b), int((bits(a) != bits(b)).any(axis=-1).sum())
    assert same(a, r), "a restart into a used sum differs from a fresh one"
    assert not same(a, full)
    other = partial_sums(*PATHS[1 - PATHS.index((side, levels))])
    assert same(a, other[0]) and same(full, other[2]), "the two ways of summing differ"


# ---- 4. spp = 1 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,levels", PATHS)
@pytest.mark.parametrize("name,w,h", [("s64", W, H), ("default", 64, 48)])
def test_one_sample_per_pixel(name, w, h, side, levels):
    """The sum after [0,1) of a 1-sample frame is rt_launch_window's binary64 slab (on the default
    scene that is the fused engine's: the sample path's wavefront frame agrees with it in exact order)."""
    win = (0, 0, w, h)
    with Ctx(scenes.named(name), side=side) as c:
        assert c.L.rt_engine(c.p, 1) == (N.RT_ENGINE_FUSED if name == "default" else N.RT_ENGINE_WAVE)
        s = Sum(c, w, h, win, DEPTH, spp=1, seed=0, levels=levels).add(0, 1)
        got, lv = s.host()
        res, _ = s.resolve("f64")
    ref, rlv = one_shot(name, w, h, win, DEPTH, "f64", 1, 0, side, levels)
    assert same(got, ref), int((bits(got) != bits(ref)).any(axis=-1).sum())
    assert same(res, ref)  # x / 1.0 is x
    assert np.array_equal(lv, rlv)


# ---- 5. partial sums against the oracle ----------------------------------------------------------
M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_position(x, y, w, h, spp, s, seed):
    """RT_SUPERSAMPLING, restated from the header."""
    r = splitmix64(seed ^ ((y * w + x) * spp + s))
    u, v = (r >> 40) * 2.0 ** -24, ((r >> 16) & 0xFFFFFF) * 2.0 ** -24
    return (x + u) / w, (y + v) / h


def test_partial_sums_against_the_oracle():
    """1000 pixels or more of S64 (every pixel whose unjittered level is >= 3 among them), spp 5: the
    oracle's colours of the sample positions restated above, summed left to right, against d_sum after
    [0,3) and [0,5).  Tolerance k * 1e-5 for k samples: the project's parity tolerance per colour
    (tests/test_gpu_knobs.py; the kernels' pow is not bit-equal to the oracle's), once per sample."""
    from oracle import oracle as O
    O.build()
    spp, seed = 5, SEED
    el = N.marshal(scenes.s64())
    olv = O.render(el, W, H, DEPTH, mode=O.MEMO, levels=True)[1]
    assert int((olv > 0).sum()) == 8344 and np.bincount(olv.ravel(), minlength=6).tolist() == [21656, 6986, 1055, 236, 47, 20]
    deep = np.flatnonzero(olv.ravel() >= 3)
    assert deep.size == 303
    rng = np.random.default_rng(5)
    hit, miss = np.flatnonzero((olv.ravel() > 0) & (olv.ravel() < 3)), np.flatnonzero(olv.ravel() == 0)
    pix = np.unique(np.concatenate([deep, rng.choice(hit, 600, replace=False), rng.choice(miss, 150, replace=False)]))
    assert pix.size >= 1000
    want3, want5, lv0 = np.zeros((pix.size, 3)), np.zeros((pix.size, 3)), np.zeros(pix.size, dtype=np.uint8)
    for i, p in enumerate(pix.tolist()):
        acc = None
        for s in range(spp):
            c, lv = O.trace_pixel(el, *sample_position(p % W, p // W, W, H, spp, s, seed), DEPTH)
            acc = np.array(c) if acc is None else acc + np.array(c)  # left to right, binary64
            if s == 0:
                lv0[i] = lv
            if s == 2:
                want3[i] = acc
        want5[i] = acc
    a, _, full, _, lv = partial_sums(None, True)
    got3, got5 = a[:H].reshape(-1, 3)[pix], full[:H].reshape(-1, 3)[pix]
    e3, e5 = float(np.abs(got3 - want3).max()), float(np.abs(got5 - want5).max())
    print(f"{pix.size} pixels: max |delta| after 3 samples {e3:.3e}, after 5 samples {e5:.3e}", flush=True)
    assert e3 <= 3 * 1e-5 and e5 <= 5 * 1e-5
    assert np.array_equal(lv[:H].ravel()[pix], lv0)


# ---- 6. several row passes -----------------------------------------------------------------------
def row_passes_child():
    """RT_QUEUE_MB=64: a queue row of S64 at 2048x96 depth 16 is 2 MB, so the slab takes three passes
    of 32 rows; the per-pass offset into the caller's d_sum on both ways of summing."""
    w, h, d, spp = 2048, 96, 16, 3
    for side, levels in PATHS:
        check_g1("s64", w, h, (0, 0, w, h), d, side=side, levels=levels, partitions=[[(0, 1), (1, 3)]], spp=spp)
    print("ok")


def test_several_row_passes():
    e = dict(os.environ, PYTHONPATH=ROOT, RT_QUEUE_MB="64")
    code = "from tests.test_gpu_progressive import row_passes_child; row_passes_child()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout.split(), r.stdout + r.stderr


# ---- 7. rt_resolve is exact ----------------------------------------------------------------------
def adversarial_sums(n, maxv):
    """Sums whose mean sits on, or one ulp either side of, a truncation boundary of maxv, and what no
    unsigned sample holds."""
    k = np.arange(0, 700, dtype=np.float64)
    mult = n * k / maxv
    small = -float(n) / maxv
    return np.concatenate([
        mult, np.nextafter(mult, -np.inf), np.nextafter(mult, np.inf), -mult,
        [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, -1.0, -2.5 * n, -1e30, 1e30, float(n), n * (1.0 - 2.0 ** -53)],
        [small, np.nextafter(small, 0.0), np.nextafter(small, -np.inf), small / 2, small * 2.0 ** -40],  # (-n/maxv, 0)
        [5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 3e-320 * n],  # binary64 subnormals
        adversarial() * n])


@functools.lru_cache(maxsize=None)
def random_sums():
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.5, 40.0, size=60000)
    x[rng.integers(0, x.size, 300)] = np.nan
    x[rng.integers(0, x.size, 300)] = np.inf
    x.setflags(write=False)
    return x


def resolve_host(x, samples, prec, maxv=255, in_off=0, out_off=0):
    """rt_resolve of the view of x from element in_off on, into a buffer that starts out_off elements
    past a 16-byte boundary, 64 guard bytes of 0xAB on each side: (values, clamped count)."""
    import torch
    dt = np.dtype(NP_DT[prec])
    n = x.size - in_off
    d = torch.from_numpy(np.array(x)).cuda()
    assert d.data_ptr() % 16 == 0
    buf = torch.full((n * dt.itemsize + 160,), 0xAB, dtype=torch.uint8, device="cuda")
    start = 64 + (out_off * dt.itemsize - (buf.data_ptr() + 64)) % 16
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    resolve_dev(d.data_ptr() + in_off * 8, n, samples, prec, maxv, buf.data_ptr() + start, cnt.data_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    end = start + n * dt.itemsize
    assert (host[:start] == 0xAB).all() and (host[end:] == 0xAB).all(), "wrote outside the output"
    return host[start:end].copy().view(dt), int(cnt.item())


def ref_resolve(x, samples, prec, maxv):
    """numpy: (values, clamped count, mask of the values to compare)."""
    with np.errstate(all="ignore"):
        m = x / float(samples)
        keep = np.ones(x.size, dtype=bool)
        if prec == "f64":
            return m, 0, keep
        if prec == "f32":
            f = m.astype(np.float32)
            # (a subnormal binary32 result is the float store's business, as in rt_launch: left out)
            keep = ~((np.abs(m) < 2.0 ** -126) & (m != 0))
            return f, 0, keep
    q, cnt = ref_quant(m, maxv, NP_DT[prec])
    return q, cnt, keep


def bytes_equal(a, b, keep):
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u)[keep], b.view(u)[keep])


@pytest.mark.parametrize("prec,maxv", [("f64", 0), ("f32", 0), ("u8", 1), ("u8", 255), ("u16", 256), ("u16", 65535)])
@pytest.mark.parametrize("samples", [1, 3, 16, 4096])
def test_resolve_is_exact(samples, prec, maxv):
    for x in (adversarial_sums(samples, maxv or 255), random_sums()):
        got, cnt = resolve_host(x, samples, prec, maxv)
        want, wcnt, keep = ref_resolve(x, samples, prec, maxv)
        assert got.dtype == want.dtype and keep.sum() >= x.size - 32
        if prec in ("f64", "f32"):  # NaN payloads: compare NaN-ness there, the bits everywhere else
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan)
            keep = keep & ~nan
        assert bytes_equal(got, want, keep), np.flatnonzero((got != want) & keep)[:8]
        assert cnt == wcnt
    if prec in ("u8", "u16"):
        assert ref_resolve(adversarial_sums(samples, maxv), samples, prec, maxv)[1] > 300


# ---- 8. rt_resolve tails and alignment -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_sums():
    rng = np.random.default_rng(22)
    x = rng.uniform(-0.25, 4.0, size=2048 * 2048 + 5 + 1)
    x[rng.integers(0, x.size, 5000)] = -1.0
    x[:4] = [-3.0, 1.5, 3.0, -0.0]
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("prec,maxv", [("f64", 0), ("f32", 0), ("u8", 255), ("u16", 65535)])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 23, 24, 2047, 2048, 2049, 2048 * 2048 + 5])
def test_resolve_tails_and_alignment(n, prec, maxv):
    """Every combination of scalar head, vector body and scalar tail, up to one value past a full pass
    of the capped grid; the sum off a 16-byte boundary (element loads), the output off one by 1 and 5
    elements (odd byte offsets for u8, 2-byte ones for u16, 4-byte ones for f32)."""
    samples = 3
    for in_off in (0, 1):
        x = big_sums()[:n + in_off]
        want, wcnt, _ = ref_resolve(x[in_off:], samples, prec, maxv)
        aligned = None
        for out_off in (0, 1, 5):
            got, cnt = resolve_host(x, samples, prec, maxv, in_off, out_off)
            if aligned is None:
                aligned = got
            assert bytes_equal(got, aligned, slice(None)), (in_off, out_off, np.flatnonzero(got != aligned)[:8])
            assert cnt == wcnt
        assert bytes_equal(aligned, want, slice(None))  # (no NaN and no subnormal in these sums)


# ---- 9. G3: an integer preview is the quantised float preview -----------------------------------
def quantize_dev(m, prec, maxv):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    out = torch.zeros(m.size, dtype={"u8": torch.uint8, "u16": torch.uint16}[prec], device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    N.check(N.lib().rt_quantize(d.data_ptr(), N.RT_OUT_F64, m.size, maxv, FMT[prec], out.data_ptr(), cnt.data_ptr(),
                                stream()), "rt_quantize")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(cnt.item())


@pytest.mark.parametrize("prec,maxv", [("u8", 255), ("u8", 7), ("u16", 65535), ("u16", 256)])
def test_integer_preview_is_the_quantised_float_preview(prec, maxv):
    part = partial_sums(0, False)[0][:H].reshape(-1)  # [0,3) of 5 samples: the preview divides by 3
    for x, samples in ((part, 3), (adversarial_sums(3, maxv), 3), (adversarial_sums(16, maxv), 16)):
        f64, _ = resolve_host(x, samples, "f64")
        got, cnt = resolve_host(x, samples, prec, maxv)
        want, wcnt = quantize_dev(f64, prec, maxv)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert cnt == wcnt
    assert cnt > 300 and got.max() == maxv


# ---- G4: a call costs its samples ------------------------------------------------------------------
def test_a_call_costs_its_samples():
    """Two samples of a 4096-sample frame launch two primary passes (the context's kernel timer counts
    k_primary's launches), and the primary masks are computed once for the frame, not per call."""
    with Ctx(scenes.s64(), side=0) as c:
        N.check(c.L.rt_configure(c.p, N.RT_CFG_KERNEL_TIMING, N.RT_KT_PRIMARY | N.RT_KT_PMASK), "rt_configure")
        s = Sum(c, W, H, (0, 0, W, H), DEPTH, spp=N.RT_MAX_SPP, levels=False).add(0, 1)
        ms, n = ctypes.c_double(0), ctypes.c_uint64(0)
        for kernel, want in ((N.RT_KT_PRIMARY, 1), (N.RT_KT_PMASK, 1)):
            N.check(c.L.rt_kernel_time(c.p, kernel, ctypes.byref(ms), ctypes.byref(n), 1), "rt_kernel_time")
            assert n.value == want, (kernel, n.value)
        s.add(1, 3)
        for kernel, want in ((N.RT_KT_PRIMARY, 2), (N.RT_KT_PMASK, 0)):
            N.check(c.L.rt_kernel_time(c.p, kernel, ctypes.byref(ms), ctypes.byref(n), 1), "rt_kernel_time")
            assert n.value == want, (kernel, n.value)
        s.host()


# ---- 10. Python -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,window", [("f64", None), ("u8", None), ("f64", WIN[:2] + (40, 30)), ("u16", (3, 5, 40, 30))])
def test_render_progressive(precision, window):
    from eraytracer_amd.raytracer import render, render_progressive
    sc = scenes.s64()
    kw = dict(spp=4, seed=SEED, precision=precision, max_value=65535 if precision == "u16" else 255, window=window)
    items = list(render_progressive(96, 64, sc, 5, steps=(1, 1, 2), **kw))
    assert [k for k, _ in items] == [1, 2, 4]
    want = render(96, 64, sc, 5, **kw)
    for _, img in items:
        assert img.shape == want.shape and img.dtype == want.dtype
    assert items[-1][1].tobytes() == want.tobytes()
    assert items[0][1].tobytes() != want.tobytes()
    assert [k for k, _ in render_progressive(96, 64, sc, 5, steps=3, **kw)] == [3, 4]


def test_progressive_frame_restart():
    import torch

    from eraytracer_amd.progressive import ProgressiveFrame
    from eraytracer_amd.raytracer import render
    with ProgressiveFrame(scenes.s64(), 96, 64, 5, spp=4, seed=SEED, levels=True) as pf:
        assert pf.samples_done == 0 and pf.add() == 1 and pf.add(2) == 3
        first = pf.resolve("f64").cpu().numpy()
        lv = pf.levels.cpu().numpy()
        assert pf.add(5) == 4 and pf.add() == 4  # clamped to what is left
        frame = pf.resolve("f32").cpu().numpy()
        u8 = pf.resolve("u8")
        assert pf.clamped() == 0 and u8.dtype == torch.uint8
        pf.restart()
        assert pf.samples_done == 0
        pf.add()
        pf.add(2)
        assert same(pf.resolve("f64").cpu().numpy(), first) and np.array_equal(pf.levels.cpu().numpy(), lv)
        pf.add()
        assert same(pf.resolve("f32").cpu().numpy(), frame)
        pf.restart(scenes.named("s16"))  # another scene in the same context
        pf.add(4)
        other = pf.resolve("f32").cpu().numpy()
    want, wlv = render(96, 64, scenes.s64(), 5, spp=4, seed=SEED, precision="f32", levels=True)
    assert frame.shape == (64, 96, 3) and same(frame, want) and np.array_equal(lv[:64], wlv)
    assert same(other, render(96, 64, scenes.named("s16"), 5, spp=4, seed=SEED, precision="f32"))

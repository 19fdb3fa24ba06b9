"""Integer frames on the GPU: rt_quantize, rt_render with precision u8 / u16, and the P6 file.

The reference of every comparison is numpy's min(trunc(x.astype(f8)*M), M) with negatives and
NaN stored as 0 (and counted), applied to the library's own binary64 frame of the same call
arguments: the oracle's frame could differ at a truncation boundary on the rare pixels where its
libm pow and the kernels' correctly rounded pow differ, so the oracle enters
only through the committed golden P3 files, which the P3 path already reproduces.  Everything is
compared byte for byte."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import records, scenes
from eraytracer_amd.raytracer import quantize_gpu, render, render_ppm_file, write_pixels_to_p6
from tests.test_int_frames import FRAMES, GOLDEN, p3_integers, p6_parts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, GRID = N.QUANT_V, N.QUANT_B, N.QUANT_MAX_BLOCKS


def ref_quant(x, maxv, dtype):
    """(samples, count of values stored as 0 because they were negative or NaN)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.trunc(x.astype(np.float64) * float(maxv))
        bad = ~(t >= 0)  # -0.0 >= 0: not counted
        q = np.where(bad, 0.0, np.minimum(t, float(maxv)))
    return q.astype(dtype), int(bad.sum())


@functools.lru_cache(maxsize=None)
def f64_frame(name, w, h, d, spp=1, seed=0, order="exact"):
    img = render(w, h, scenes.named(name), d, spp=spp, seed=seed, order=order)
    img.setflags(write=False)
    return img


def adversarial():
    k = np.arange(0, 600, dtype=np.float64)
    tiny = np.array([5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310])
    return np.concatenate([k / 255.0, (k + 0.5) / 255.0, -k / 255.0, np.nextafter(k / 255.0, -1.0),
                           [0.0, -0.0, 1.0, 2.0, 1e30, -1e5, 254.999999999 / 255.0, 1.0 - 1e-17],
                           [np.inf, np.nan, -np.inf, -np.nan], tiny,
                           -1.0 / np.array([1, 7, 255, 256, 65535.0]),
                           np.nextafter(-1.0 / np.array([255.0, 65535.0]), 0.0), k / 65535.0,
                           (k * 109 + 0.5) / 65535.0])


@pytest.mark.parametrize("dt_out,maxv", [(np.uint8, 1), (np.uint8, 7), (np.uint8, 255), (np.uint16, 256),
                                         (np.uint16, 65535)])
@pytest.mark.parametrize("dt_in", [np.float64, np.float32])
def test_quantize_is_exact(dt_in, dt_out, maxv):
    with np.errstate(over="ignore"):
        vals = adversarial().astype(dt_in)  # binary32: the reference starts from the rounded values
        frame = f64_frame("s64", 48, 40, 5).astype(dt_in)
    for x in (vals, frame):
        got, cnt = quantize_gpu(x, maxv, dt_out)
        want, wcnt = ref_quant(x, maxv, dt_out)
        assert got.dtype == np.dtype(dt_out) and got.shape == x.shape
        assert np.array_equal(got, want), np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8]
        assert cnt == wcnt
    assert ref_quant(vals, maxv, dt_out)[1] > 300  # negatives at or below -1/maxv, NaN and -inf were counted


@functools.lru_cache(maxsize=None)
def random_values():
    rng = np.random.default_rng(20)
    x = rng.uniform(-0.25, 1.25, size=GRID * B + 4 * B)
    x[rng.integers(0, x.size, 5000)] = np.nan
    x[rng.integers(0, x.size, 5000)] = np.inf
    x[[0, 1, 2, 3]] = [-1.0, 0.5, np.nan, -0.0]
    x.setflags(write=False)
    return x


def quantize_at(x, in_off, out_off, maxv, dt_out):
    """rt_quantize on the view of x that starts at element in_off, into a device buffer at
    byte offset out_off from a 16-byte boundary, with 64 guard bytes of 0xAB on each side:
    (samples, count, guards intact)."""
    import torch
    dt = np.dtype(dt_out)
    n = x.size - in_off
    prec = N.RT_OUT_F64 if x.dtype == np.float64 else N.RT_OUT_F32
    d = torch.from_numpy(np.array(x)).cuda()
    buf = torch.full((n * dt.itemsize + 160,), 0xAB, dtype=torch.uint8, device="cuda")
    start = 64 + (out_off - (buf.data_ptr() + 64)) % 16
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    N.check(N.lib().rt_quantize(d.data_ptr() + in_off * x.dtype.itemsize, prec, n, maxv,
                                N.RT_OUT_U8 if dt == np.uint8 else N.RT_OUT_U16, buf.data_ptr() + start,
                                cnt.data_ptr(), torch.cuda.current_stream().cuda_stream), "rt_quantize")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    end = start + n * dt.itemsize
    guards = bool((host[:start] == 0xAB).all() and (host[end:] == 0xAB).all())
    return host[start:end].copy().view(dt), int(cnt.item()), guards


SIZES = [1, 2, 3, V - 1, V, V + 1, B - 1, B, B + 1, 3 * B + 7, GRID * B + B + 5]


@pytest.mark.parametrize("n", SIZES)
def test_quantize_sizes_hit_every_tail(n):
    """One value to one past a full pass of the capped grid (the stride loop's second, partial
    pass): every combination of scalar head, vector body and scalar tail."""
    x = random_values()[:n]
    for src, dt_out, maxv, out_off in ((x, np.uint8, 255, 0), (x.astype(np.float32), np.uint16, 65535, 0),
                                       (x, np.uint8, 7, 5)):
        got, cnt, guards = quantize_at(src, 0, out_off, maxv, dt_out)
        want, wcnt = ref_quant(src, maxv, dt_out)
        assert guards
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert cnt == wcnt


@pytest.mark.parametrize("dt_out,out_off", [(np.uint8, 0), (np.uint8, 1), (np.uint8, 3), (np.uint8, 15),
                                            (np.uint16, 0), (np.uint16, 2)])
@pytest.mark.parametrize("in_off", [0, 1])
@pytest.mark.parametrize("dt_in", [np.float64, np.float32])
def test_quantize_alignment_and_guards(dt_in, in_off, dt_out, out_off):
    """Element-aligned input (element 1 is not 16-byte aligned) and any output alignment; the 64
    bytes on each side of the output stay as they were."""
    maxv = 255 if dt_out == np.uint8 else 65535
    for n in (3 * B + 7, 11):
        x = random_values()[: n + in_off].astype(dt_in)
        got, cnt, guards = quantize_at(x, in_off, out_off, maxv, dt_out)
        want, wcnt = ref_quant(x[in_off:], maxv, dt_out)
        assert guards
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert cnt == wcnt


# ---- rt_render with integer output ---------------------------------------------------------
INT = [("u8", 255, np.uint8), ("u16", 65535, np.uint16)]


@pytest.mark.parametrize("prec,maxv,dt", INT)
@pytest.mark.parametrize("name,w,h", [("default", 64, 48), ("s64", 96, 80), ("mixed", 96, 64)])
def test_render_integer_equals_quantised_f64(name, w, h, prec, maxv, dt):
    want, _ = ref_quant(f64_frame(name, w, h, 5), maxv, dt)
    st = {}
    got = render(w, h, scenes.named(name), 5, precision=prec, max_value=maxv, stats=st)  # pageable
    assert got.dtype == np.dtype(dt) and got.shape == (h, w, 3)
    assert np.array_equal(got, want) and st["clamped"] is False and st["pinned"] is False
    out = N.pinned_empty((h, w, 3), dt)
    out[:] = 0x5A
    assert render(w, h, scenes.named(name), 5, precision=prec, max_value=maxv, out=out, stats=st) is out
    assert np.array_equal(out, want) and st["clamped"] is False and st["pinned"] is True
    with pytest.raises(ValueError):
        render(w, h, scenes.named(name), 5, precision=prec, out=np.empty((h, w, 3), np.float32))


def test_render_integer_max_value_default_and_limits():
    want, _ = ref_quant(f64_frame("default", 64, 48, 5), 255, np.uint8)
    assert np.array_equal(render(64, 48, scenes.named("default"), 5, precision="u8"), want)
    want7, _ = ref_quant(f64_frame("default", 64, 48, 5), 7, np.uint16)
    assert np.array_equal(render(64, 48, scenes.named("default"), 5, precision="u16", max_value=7), want7)
    for prec, maxv in (("u8", 256), ("u16", 65536)):
        with pytest.raises(N.RtError) as ei:
            render(64, 48, scenes.named("default"), 5, precision=prec, max_value=maxv)
        assert ei.value.code == N.RT_ETOOBIG
    # a struct_size that ends before max_value (an older caller) selects 255
    el = N.marshal(scenes.named("default"))
    opts = N.RtOpts(N.RtOpts.max_value.offset, 0, 1, N.RT_OUT_U8, N.RT_ORDER_EXACT, 16, None, 1, 0, 0, 0, 9)
    out = np.empty((48, 64, 3), np.uint8)
    N.check(N.lib().rt_render(el, len(el), 64, 48, 5, ctypes.byref(opts), out.ctypes.data, None), "rt_render")
    assert np.array_equal(out, want)


@pytest.mark.parametrize("prec,maxv,dt", INT)
def test_render_integer_spp_and_fast_order(prec, maxv, dt):
    sc = scenes.named("s64")
    want, _ = ref_quant(f64_frame("s64", 96, 80, 5, 3, 9), maxv, dt)
    assert np.array_equal(render(96, 80, sc, 5, precision=prec, max_value=maxv, spp=3, seed=9), want)
    want, _ = ref_quant(f64_frame("s64", 96, 80, 5, 1, 0, "fast"), maxv, dt)
    assert np.array_equal(render(96, 80, sc, 5, precision=prec, max_value=maxv, order="fast"), want)


@pytest.mark.parametrize("prec,maxv,dt", INT)
def test_render_integer_shards_and_levels(prec, maxv, dt):
    """Three shards of 16-row blocks at 70 rows (the last block is ragged, and shard 2's slab has
    rows past the image, which are neither quantised nor counted) give the one-shard frame; the
    primary-hit mask is what the float frame's call returns."""
    sc = scenes.named("s64")
    st = {}
    one = render(96, 70, sc, 5, precision=prec, max_value=maxv)
    assert np.array_equal(one, ref_quant(f64_frame("s64", 96, 70, 5), maxv, dt)[0])
    for out in (None, N.pinned_empty((70, 96, 3), dt)):
        got = render(96, 70, sc, 5, precision=prec, max_value=maxv, nshards=3, row_block=16, stats=st, out=out)
        assert np.array_equal(got, one) and st["clamped"] is False
    _, lv = render(96, 80, sc, 5, levels="hit")
    img, ilv = render(96, 80, sc, 5, precision=prec, max_value=maxv, levels="hit")
    assert np.array_equal(ilv, lv) and 0 < int(lv.sum()) < lv.size
    assert np.array_equal(img, ref_quant(f64_frame("s64", 96, 80, 5), maxv, dt)[0])


_BANDS_CHILD = r"""
import numpy as np
from eraytracer_amd import _native as N, scenes
from eraytracer_amd.raytracer import render
from tests.test_gpu_int_frames import ref_quant
w, h, sc = 2048, 424, scenes.named('s64')
f64 = render(w, h, sc, 2)
for prec, maxv, dt in (('u8', 255, np.uint8), ('u16', 65535, np.uint16)):
    want, _ = ref_quant(f64, maxv, dt)
    for out in (None, N.pinned_empty((h, w, 3), dt)):
        st = {}
        got = render(w, h, sc, 2, precision=prec, max_value=maxv, out=out, stats=st)
        assert st['pinned'] is (out is not None) and st['clamped'] is False
        assert np.array_equal(got, want), (prec, out is None, int((got != want).sum()))
print('ok')
"""


def test_render_integer_over_several_row_bands():
    """RT_BAND_MB=1 (read once per process: a child): bands are sized on the bytes copied, so a
    2048x424 frame takes 3 bands of 8-bit rows (160, 160, 104) and 6 of 16-bit rows (5 x 80, 24),
    the last one shorter and ending inside a 16-row tile — pinned and pageable destinations."""
    for esz in (1, 2):  # rt_render's band rule: whole 16-row tiles, about RT_BAND_MB of output each
        rowbytes = 2048 * 3 * esz
        band = max((1 << 20) // rowbytes // 16 * 16, 16)
        assert -(-424 // band) >= 3 and 424 % band != 0
    e = dict(os.environ, PYTHONPATH=ROOT, RT_BAND_MB="1")
    r = subprocess.run([sys.executable, "-c", _BANDS_CHILD], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout.split(), r.stdout + r.stderr


def huge_scene():
    return records.scene()[:2] + [records.sphere(4, records.vector(4, 0, 10),
                                                 records.material(records.colour(-1e12, 0.5, 1), 20, 1, 0.1))]


def test_clamp_flag_and_p6_range_error(tmp_path):
    sc = huge_scene()
    f64 = render(24, 18, sc, 3)
    want, wcnt = ref_quant(f64, 255, np.uint8)
    assert wcnt > 0
    st = {}
    got = render(24, 18, sc, 3, precision="u8", stats=st)
    assert st["clamped"] is True and np.array_equal(got, want)
    assert quantize_gpu(f64, 255, np.uint8)[1] == wcnt
    out = tmp_path / "huge.ppm"
    with pytest.raises(N.RtError) as ei:
        render_ppm_file(24, 18, sc, 3, str(out), binary=True)
    assert ei.value.code == N.RT_ERANGE and not out.exists()
    render(64, 48, records.scene(), 5, precision="u8", stats=st)
    assert st["clamped"] is False


@pytest.mark.parametrize("name,w,h", FRAMES)
def test_p6_file_matches_the_golden_p3_files(tmp_path, name, w, h):
    out = tmp_path / name
    assert render_ppm_file(w, h, records.scene(), 1, str(out), binary=True) == "ok"
    head, body = p6_parts(out.read_bytes())
    assert head == f"P6\n{w} {h}\n255\n".encode()
    assert list(body) == p3_integers(open(os.path.join(GOLDEN, name), "rb").read())[3]


@pytest.mark.parametrize("maxv", [255, 1000])
def test_p6_file_matches_the_host_writer(tmp_path, maxv):
    got, want = tmp_path / "gpu.ppm", tmp_path / "host.ppm"
    assert render_ppm_file(56, 40, scenes.s64(), 5, str(got), max_value=maxv, binary=True) == "ok"
    write_pixels_to_p6(56, 40, maxv, f64_frame("s64", 56, 40, 5), str(want))
    assert got.read_bytes() == want.read_bytes()
    assert len(p6_parts(got.read_bytes())[1]) == 56 * 40 * 3 * (2 if maxv > 255 else 1)

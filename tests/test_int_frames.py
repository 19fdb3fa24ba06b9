"""Integer frames on the CPU: the host P6 writer (write_pixels_to_p6, the reference the GPU
tests compare against) on the oracle's frames against the committed golden P3 files, its edge
cases, the argument checks of rt_quantize and rt_render_rawppm_file (made before any HIP call, so
no device is needed), and the layout of the field appended to rt_opts."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import records
from eraytracer_amd.raytracer import write_pixels_to_p6, write_pixels_to_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FRAMES = (("run_sh_32x24_d1.ppm", 32, 24), ("run_concurrent_sh_16x12_d1.ppm", 16, 12))


def p3_integers(data: bytes):
    """(W, H, MaxValue, integers) of a P3 file."""
    magic, size, maxv, body = data.split(b"\n", 3)
    assert magic == b"P3"
    w, h = map(int, size.split())
    return w, h, int(maxv), [int(t) for t in body.split()]


def p6_parts(data: bytes):
    """(header bytes, payload bytes) of a P6 file."""
    k = 0
    for _ in range(3):
        k = data.index(b"\n", k) + 1
    return data[:k], data[k:]


@pytest.mark.parametrize("name,w,h", FRAMES)
def test_p6_writer_matches_the_golden_p3_files(oracle, tmp_path, name, w, h):
    img = oracle.render(N.marshal(records.scene()), w, h, 1, mode=oracle.MEMO)
    gw, gh, gmax, want = p3_integers(open(os.path.join(GOLDEN, name), "rb").read())
    assert (gw, gh, gmax) == (w, h, 255)
    out = tmp_path / "a.ppm"
    write_pixels_to_p6(w, h, 255, img, str(out))
    head, body = p6_parts(out.read_bytes())
    assert head == f"P6\n{w} {h}\n255\n".encode()
    assert len(body) == w * h * 3 and list(body) == want
    # the pixel list form gives the same file
    pixels = [(1, tuple(px)) for px in img.reshape(-1, 3).tolist()]
    out2 = tmp_path / "b.ppm"
    write_pixels_to_p6(w, h, 255, pixels, str(out2))
    assert out2.read_bytes() == out.read_bytes()


@pytest.mark.parametrize("name,w,h", FRAMES)
def test_p6_writer_16_bit_samples_are_big_endian_and_match_p3(oracle, tmp_path, name, w, h):
    img = oracle.render(N.marshal(records.scene()), w, h, 1, mode=oracle.MEMO)
    p3 = tmp_path / "a.p3"
    write_pixels_to_ppm(w, h, 65535, img, str(p3))
    _, _, maxv, want = p3_integers(p3.read_bytes())
    assert maxv == 65535 and max(want) > 255
    out = tmp_path / "a.p6"
    write_pixels_to_p6(w, h, 65535, img, str(out))
    head, body = p6_parts(out.read_bytes())
    assert head == f"P6\n{w} {h}\n65535\n".encode()
    assert len(body) == w * h * 6
    assert [body[i] << 8 | body[i + 1] for i in range(0, len(body), 2)] == want


def test_p6_writer_edge_cases(tmp_path):
    out = tmp_path / "x.ppm"
    with pytest.raises(ValueError):
        write_pixels_to_p6(1, 1, 255, [(1, (2.5, -0.4, 0))], str(out))
    with pytest.raises(ValueError):
        write_pixels_to_p6(1, 1, 255, np.array([[[2.5, -0.4, 0.0]]]), str(out))
    with pytest.raises(ValueError):
        write_pixels_to_p6(1, 1, 255, np.array([[[0.5, float("nan"), 0.0]]]), str(out))
    assert not out.exists()                                  # nothing is opened before the check
    write_pixels_to_p6(2, 1, 255, [(1, (2.5, -0.0, 0)), (1, (float("inf"), -0.0039, 1.0))], str(out))
    assert p6_parts(out.read_bytes())[1] == bytes([255, 0, 0, 255, 0, 255])  # -0.0039*255 = -0.99: trunc 0
    write_pixels_to_p6(1, 1, 1000, np.array([[[2.5, -0.0, 0.5]]], dtype=np.float32), str(out))
    assert p6_parts(out.read_bytes())[1] == bytes([0x03, 0xE8, 0, 0, 0x01, 0xF4])
    for bad in (0, 65536, 2.0, True):
        with pytest.raises(ValueError):
            write_pixels_to_p6(1, 1, bad, [(1, (0, 0, 0))], str(out))


def test_quantize_argument_checks_need_no_device(native):
    L = native.lib()
    a, b = 0x1000, 0x2000  # never dereferenced: every case below fails its checks
    q = L.rt_quantize
    assert q(None, N.RT_OUT_F64, 8, 255, N.RT_OUT_U8, b, None, None) == N.RT_EBADARG
    assert q(a, N.RT_OUT_F64, 8, 255, N.RT_OUT_U8, None, None, None) == N.RT_EBADARG
    assert q(a, N.RT_OUT_U8, 8, 255, N.RT_OUT_U8, b, None, None) == N.RT_EBADARG      # precision
    assert q(a, N.RT_OUT_F64, 8, 255, N.RT_OUT_F32, b, None, None) == N.RT_EBADARG    # out_format
    assert q(a, N.RT_OUT_F64, 8, 255, 4, b, None, None) == N.RT_EBADARG
    assert q(a, N.RT_OUT_F64, 8, 0, N.RT_OUT_U8, b, None, None) == N.RT_EBADARG
    assert q(a, N.RT_OUT_F32, 8, 0, N.RT_OUT_U16, b, None, None) == N.RT_EBADARG
    assert q(a, N.RT_OUT_F64, 8, 256, N.RT_OUT_U8, b, None, None) == N.RT_ETOOBIG
    assert q(a, N.RT_OUT_F32, 8, 65536, N.RT_OUT_U16, b, None, None) == N.RT_ETOOBIG
    assert q(a + 4, N.RT_OUT_F64, 8, 255, N.RT_OUT_U8, b, None, None) == N.RT_EBADARG  # element alignment
    assert q(a, N.RT_OUT_F64, 8, 255, N.RT_OUT_U16, b + 1, None, None) == N.RT_EBADARG
    assert q(a, N.RT_OUT_F64, 0, 255, N.RT_OUT_U8, b, None, None) == N.RT_OK          # nothing launched
    assert q(a + 4, N.RT_OUT_F32, 0, 65535, N.RT_OUT_U16, b + 2, None, None) == N.RT_OK


def test_render_p6_file_argument_checks_need_no_device(native, tmp_path):
    L = native.lib()
    el = N.marshal(records.scene())
    path = str(tmp_path / "never.ppm").encode()
    assert L.rt_render_rawppm_file(el, len(el), 4, 3, 1, None, 255, None, None) == N.RT_EBADARG
    assert L.rt_render_rawppm_file(el, len(el), 0, 0, 1, None, 255, path, None) == N.RT_DONE
    assert L.rt_render_rawppm_file(el, len(el), 4, 0, 1, None, 255, path, None) == N.RT_EBADARG
    assert L.rt_render_rawppm_file(el, len(el), 4, 3, 1, None, 70000, path, None) == N.RT_ETOOBIG
    assert L.rt_render_rawppm_file(el, len(el), 4, 3, 1, None, 0, path, None) == N.RT_EBADARG
    assert not os.path.exists(path.decode())


def test_constants_match_the_header_and_the_kernel():
    src = open(HEADER).read()
    for name in ("RT_OUT_U8", "RT_OUT_U16", "RT_MAX_INT_VALUE", "RT_STATS_PINNED", "RT_STATS_CLAMPED"):
        m = re.search(rf"#define\s+{name}\s+(\d+)", src)
        assert m and int(m.group(1)) == getattr(N, name), name
    k = open(os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_quant.hip")).read()
    block = int(re.search(r"QUANT_BLOCK = (\d+);", k).group(1))
    assert int(re.search(r"QUANT_V = (\d+);", k).group(1)) == N.QUANT_V
    assert block * N.QUANT_V == N.QUANT_B
    assert int(re.search(r"QUANT_MAX_BLOCKS = (\d+);", k).group(1)) == N.QUANT_MAX_BLOCKS
    assert {"rt_quantize", "rt_render_rawppm_file"} <= set(N.EXPORTS)
    for name in ("rt_quantize", "rt_render_rawppm_file"):
        assert re.search(rf"\bint {name}\(", src), name


def test_opts_max_value_layout_matches_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_mi355x.h"
int main(void){printf("%zu %zu %zu %zu\n", sizeof(rt_opts), offsetof(rt_opts, flags), offsetof(rt_opts, max_value),
 sizeof(rt_stats)); return 0;}
'''
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [ctypes.sizeof(N.RtOpts), N.RtOpts.flags.offset, N.RtOpts.max_value.offset, ctypes.sizeof(N.RtStats)]
    assert N.RtOpts.max_value.size == 4

"""Pixel windows (RT_WINDOW in include/rt_mi355x.h) on the CPU: the layout of the four fields
appended to rt_opts, the header's contract, the window checks of rt_render, the file writers and
rt_launch_window (made before the scene check and before any HIP call, so no device is needed), and
the checks of raytracer.render(window=...), made before the library is loaded."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
FIELDS = ("win_x0", "win_y0", "win_w", "win_h")
W, H = 200, 150
# (x0, y0, w, h) that rt_render must refuse for a 200x150 image
BAD_WINDOWS = {
    "zero width": (0, 0, 0, 10),
    "zero height": (0, 0, 10, 0),
    "origin with a zero size": (5, 0, 0, 0),
    "row origin with a zero size": (0, 7, 0, 0),
    "leaves on the right": (150, 0, 51, 10),
    "leaves at the bottom": (0, 100, 10, 51),
    "origin outside": (200, 0, 1, 1),
    "sum wraps in 32 bits": (0xFFFFFFF0, 0, 0x20, 1),
}


def test_opts_window_layout_matches_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_mi355x.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rt_opts), offsetof(rt_opts, max_value),
 offsetof(rt_opts, win_x0), offsetof(rt_opts, win_y0), offsetof(rt_opts, win_w), offsetof(rt_opts, win_h)); return 0;}
'''
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [ctypes.sizeof(N.RtOpts), N.RtOpts.max_value.offset] + [getattr(N.RtOpts, f).offset for f in FIELDS]
    assert all(getattr(N.RtOpts, f).size == 4 for f in FIELDS)
    # appended: the fields follow max_value, in the header's order
    assert [getattr(N.RtOpts, f).offset for f in FIELDS] == [N.RtOpts.max_value.offset + 4 * (i + 1) for i in range(4)]
    # the positional constructors that predate the fields still build a whole-frame block
    o = N.RtOpts(ctypes.sizeof(N.RtOpts), 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, 16, None, 1, 0, 0, 0, 255)
    assert (o.win_x0, o.win_y0, o.win_w, o.win_h) == (0, 0, 0, 0)


def test_header_contract():
    src = open(HEADER).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    m = re.search(r"\bint rt_launch_window\(([^;]*)\);", src)
    assert m, "the header does not declare rt_launch_window"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "p", "width", "height", "depth", "x0", "y0", "win_w", "win_h", "row_block", "shard", "nshards", "precision",
        "order", "spp", "seed", "d_out", "d_levels", "stream"]
    assert "rt_launch_window" in N.EXPORTS and not any(ch.isdigit() for ch in "rt_launch_window")
    assert re.search(r"uint32_t win_x0, win_y0, win_w, win_h;", src)
    assert src.index("uint32_t max_value;") < src.index("uint32_t win_x0")
    assert "hipMemcpy2DAsync" in src  # the packed-to-pitched copy is named as the caller's


def opts_with(window, struct_size=None):
    o = N.RtOpts(struct_size or ctypes.sizeof(N.RtOpts), 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, 16, None, 1, 0, 0, 0, 255,
                 *window)
    return o


@pytest.mark.parametrize("what", sorted(BAD_WINDOWS))
def test_render_refuses_a_bad_window_before_the_scene_and_any_hip_call(native, what):
    L = native.lib()
    el = N.marshal(records.scene())
    out = np.full((H, W, 3), 7.0)
    o = opts_with(BAD_WINDOWS[what])
    assert L.rt_render(el, len(el), W, H, 1, ctypes.byref(o), out.ctypes.data, None) == N.RT_EBADARG
    # ... before the scene check: a scene check_scene refuses (no elements) still reports the window
    assert L.rt_render(el, 0, W, H, 1, ctypes.byref(o), out.ctypes.data, None) == N.RT_EBADARG
    assert np.all(out == 7.0)


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="checks the no-device path")
def test_render_accepts_a_valid_window_then_looks_for_a_device(native):
    """The window checks come first: on a machine without a device a valid window gets as far as
    RT_ENODEV, and so does a block whose struct_size ends before the fields, whatever follows it.
    (With a device the valid windows are rendered: tests/test_gpu_window.py.)"""
    L = native.lib()
    el = N.marshal(records.scene())
    out = np.zeros((H, W, 3))
    for win in ((37, 21, 83, 59), (0, 0, W, H), (199, 149, 1, 1), (0, 0, 0, 0)):
        o = opts_with(win)
        assert L.rt_render(el, len(el), W, H, 1, ctypes.byref(o), out.ctypes.data, None) == N.RT_ENODEV, win
    o = opts_with((0, 0, 0, 10), struct_size=N.RtOpts.win_x0.offset)  # the fields lie past struct_size: not read
    assert L.rt_render(el, len(el), W, H, 1, ctypes.byref(o), out.ctypes.data, None) == N.RT_ENODEV


def test_file_writers_refuse_a_bad_window(native, tmp_path):
    L = native.lib()
    el = N.marshal(records.scene())
    path = str(tmp_path / "never.ppm").encode()
    for what, win in sorted(BAD_WINDOWS.items()):
        o = opts_with(win)
        assert L.rt_render_ppm_file(el, len(el), W, H, 1, ctypes.byref(o), 255, path, None) == N.RT_EBADARG, what
        assert L.rt_render_rawppm_file(el, len(el), W, H, 1, ctypes.byref(o), 255, path, None) == N.RT_EBADARG, what
    assert not os.path.exists(path.decode())


def test_launch_window_argument_checks_need_no_device(native):
    lw = native.lib().rt_launch_window
    a = 0x1000  # never dereferenced
    f64, ex = N.RT_OUT_F64, N.RT_ORDER_EXACT
    assert lw(None, W, H, 5, 37, 21, 83, 59, 16, 0, 1, f64, ex, 1, 0, a, None, None) == N.RT_EBADARG
    assert lw(None, W, H, 5, 0, 0, W, H, 16, 0, 1, f64, ex, 1, 0, a, None, None) == N.RT_EBADARG


@pytest.mark.parametrize("window", [(0, 0, 0, 10), (0, 0, 10, 0), (5, 0, 0, 0), (150, 0, 51, 10), (0, 100, 10, 51),
                                    (-1, 0, 10, 10), (0, -1, 10, 10), (0, 0, 10), (0, 0, 10.0, 10), "abcd", (0, 0, True, 1)])
def test_python_render_refuses_a_bad_window_without_the_library(monkeypatch, tmp_path, window):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(N, "lib", boom)
    with pytest.raises(ValueError):
        raytracer.render(W, H, records.scene(), 1, window=window)
    with pytest.raises(ValueError):
        raytracer.render_ppm_file(W, H, records.scene(), 1, str(tmp_path / "never.ppm"), window=window)
    assert not (tmp_path / "never.ppm").exists()


def test_python_render_checks_out_against_the_window_without_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(N, "lib", boom)
    win = (37, 21, 83, 59)
    for bad in (np.zeros((H, W, 3)), np.zeros((83, 59, 3)), np.zeros((59, 83, 3), dtype=np.float32),
                np.zeros((59, 83, 4))[:, :, :3]):
        with pytest.raises(ValueError):
            raytracer.render(W, H, records.scene(), 1, window=win, out=bad)
    # the right shape passes the checks and reaches the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.render(W, H, records.scene(), 1, window=win, out=np.zeros((59, 83, 3)))
    # without a window `out` is still the frame's
    with pytest.raises(ValueError):
        raytracer.render(W, H, records.scene(), 1, out=np.zeros((59, 83, 3)))

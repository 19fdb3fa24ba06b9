"""rt_query_colours and the aimed camera (RT_QUERY in include/rt_mi355x.h) on the CPU: the header's
declarations, the argument checks and the size function (all made before any HIP call and before the
context is read, so no device is needed), the same under the host sanitizers in a stand-alone program,
raytracer.view_rays, the checks of raytracer.trace_rays (made before the library is loaded), and the
population of the batches tests/test_gpu_trace.py sends, on the reference alone: the GPU comparisons
cannot pass on empty ground."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer, records
from tests import query_ref as Q
from tests import trace_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
A16 = 0x10000  # a pointer never dereferenced, aligned for everything
REC = 76       # bytes per ray and level: nine doubles and an int


def test_header_declares_the_call_and_its_size_function():
    src = open(HEADER).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    want = {"rt_query_colours_work_bytes": ("size_t", ["n", "depth"]),
            "rt_query_colours": ("int", ["p", "d_origin", "d_dir", "n", "depth", "flags", "precision", "d_rgb", "d_levels",
                                         "d_work", "work_bytes", "stream"])}
    for name, (ret, names) in want.items():
        m = re.search(r"\b%s %s\(([^;]*)\);" % (ret, name), src)
        assert m, f"the header does not declare {name}"
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
        assert name in N.EXPORTS and not any(ch.isdigit() for ch in name)
    assert "rt_query_colours" in src[src.index("/* RT_QUERY"):src.index("#define RT_QUERY_ONE_ORIGIN")]


def colours(L, *, p=A16, o=A16, d=A16, n=100, depth=3, flags=0, prec=N.RT_OUT_F64, rgb=A16, levels=None, work=A16,
            work_bytes=None):
    if work_bytes is None:
        work_bytes = L.rt_query_colours_work_bytes(n, depth) if n <= N.RT_MAX_QUERY_RAYS else 1 << 62
    return L.rt_query_colours(p, o, d, n, depth, flags, prec, rgb, levels, work, work_bytes, None)


def test_argument_checks_need_no_device_and_never_read_the_context(native):
    """Every documented argument error, with a context pointer that is null or would fault if read."""
    L = native.lib()
    bad, big = N.RT_EBADARG, N.RT_ETOOBIG
    for name in ("p", "o", "d", "rgb"):
        assert colours(L, **{name: None}) == bad, name
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert colours(L, flags=flags) == bad, flags
    for prec in (N.RT_OUT_U8, N.RT_OUT_U16, -1, 4):
        assert colours(L, prec=prec) == bad, prec
    for off in (1, 2, 4):
        assert colours(L, o=A16 + off) == bad and colours(L, d=A16 + off) == bad
    assert colours(L, rgb=A16 + 4) == bad and colours(L, rgb=A16 + 2, prec=N.RT_OUT_F32) == bad
    assert colours(L, work=None) == bad
    for off in (1, 4, 8):
        assert colours(L, work=A16 + off) == bad, off
    need = L.rt_query_colours_work_bytes(100, 3)
    assert need > 0 and colours(L, work_bytes=need - 1) == bad and colours(L, work_bytes=0) == bad
    for n in (N.RT_MAX_QUERY_RAYS + 1, 1 << 40, (1 << 64) - 1):
        assert colours(L, n=n) == big, n
    # a size that overflows size_t: 2^30 rays at depth 2^32 - 1
    assert L.rt_query_colours_work_bytes(N.RT_MAX_QUERY_RAYS, 0xFFFFFFFF) == 0
    assert colours(L, n=N.RT_MAX_QUERY_RAYS, depth=0xFFFFFFFF, work_bytes=(1 << 64) - 1) == big
    # RT_EBADARG comes before RT_ETOOBIG
    for n, depth in ((N.RT_MAX_QUERY_RAYS + 1, 3), (N.RT_MAX_QUERY_RAYS, 0xFFFFFFFF)):
        kw = dict(n=n, depth=depth, work_bytes=(1 << 64) - 1)
        assert colours(L, p=None, **kw) == bad and colours(L, flags=2, **kw) == bad
        assert colours(L, prec=7, **kw) == bad and colours(L, d=A16 + 4, **kw) == bad and colours(L, rgb=A16 + 1, **kw) == bad


def test_nothing_to_do_launches_nothing(native):
    """n = 0 is RT_OK with a context that would fault if read and a null work space — and still an error
    with bad arguments."""
    L = native.lib()
    assert colours(L, n=0, work=None, work_bytes=0) == N.RT_OK
    assert colours(L, n=0, work=None, work_bytes=0, flags=1, prec=N.RT_OUT_F32, rgb=A16 + 4, levels=A16 + 1) == N.RT_OK
    assert colours(L, n=0, p=None) == N.RT_EBADARG and colours(L, n=0, flags=2) == N.RT_EBADARG
    assert colours(L, n=0, rgb=None) == N.RT_EBADARG


def test_work_bytes(native):
    wb = native.lib().rt_query_colours_work_bytes
    assert wb(0, 5) == 0 and wb(5, 0) == 0 and wb(0, 0) == 0
    assert wb(1, 1) == 64 * REC and wb(64, 1) == 64 * REC and wb(65, 2) == 2 * 128 * REC
    for depth in (1, 3, 40):
        sizes = [wb(n, depth) for n in range(0, 300)]
        assert sizes == sorted(sizes) and all(s >= n * depth * REC for n, s in enumerate(sizes))
    for n in (1, 63, 4133):
        sizes = [wb(n, d) for d in range(0, 50)]
        assert sizes == sorted(sizes) and sizes[1] > 0
    assert wb(N.RT_MAX_QUERY_RAYS, 5) == (1 << 30) * REC * 5
    assert wb(N.RT_MAX_QUERY_RAYS, 226050910) > 0 and wb(N.RT_MAX_QUERY_RAYS, 226050911) == 0  # 2^64 / (76 2^30)
    assert wb((1 << 64) - 1, 1) == 0


def test_size_function_and_checks_under_host_sanitizers(tmp_path):
    """rt_trace_args.h — the size function and every argument check — in a stand-alone program built with
    AddressSanitizer + UBSan: a sweep of (n, depth) across the overflow edge of size_t."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "trace_args_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "trace_args_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout) >= 1000


# ---- view_rays -----------------------------------------------------------------------------------
def test_view_rays_is_a_look_at_pinhole_camera():
    eye, target, up = (3.0, 2.0, -6.0), (0.0, 0.0, 10.0), (0.0, 1.0, 0.0)
    w, h, fov = 8, 6, 70
    e, d = raytracer.view_rays(w, h, eye, target, up, fov)
    assert e.dtype == d.dtype == np.float64 and e.shape == (3,) and d.shape == (h * w, 3) and d.flags.c_contiguous
    assert np.array_equal(e, np.array(eye))
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 4e-16
    fwd = (np.array(target) - e) / np.linalg.norm(np.array(target) - e)
    img = d.reshape(h, w, 3)
    # pixel (W/2, H/2) is (x/W - 0.5, y/H - 0.5) = (0, 0): fwd itself; the centre of the even frame straddles it
    assert np.abs(img[h // 2, w // 2] - fwd).max() <= 4e-16
    # the axes, recovered from the image: orthogonal, unit, right-handed as documented
    right = img[h // 2, w // 2 + 1] / (img[h // 2, w // 2 + 1] @ fwd) - fwd
    down = img[h // 2 + 1, w // 2] / (img[h // 2 + 1, w // 2] @ fwd) - fwd
    hw = np.tan(np.radians(fov) / 2)
    assert abs(np.linalg.norm(right) - 2 * hw / w) <= 1e-14 and abs(np.linalg.norm(down) - 2 * hw * (h / w) / h) <= 1e-14
    r, dn = right / np.linalg.norm(right), down / np.linalg.norm(down)
    assert abs(r @ fwd) <= 1e-14 and abs(dn @ fwd) <= 1e-14 and abs(r @ dn) <= 1e-14
    assert np.abs(np.cross(fwd, r) - dn).max() <= 1e-13
    assert np.abs(r - np.cross(up, fwd) / np.linalg.norm(np.cross(up, fwd))).max() <= 1e-13
    # (as in the reference, pixel x sits at x/W: the pixels before the centre one lie on the other side of fwd)
    assert img[h // 2, w // 2 - 1] @ r < 0 < img[h // 2, w // 2 + 1] @ r
    assert img[h // 2 - 1, w // 2] @ dn < 0 < img[h // 2 + 1, w // 2] @ dn
    # the left edge of row y is -hw along right: tan of the half angle
    left = img[h // 2, 0]
    assert abs(np.arctan2(-(left @ r), left @ fwd) - np.radians(fov) / 2) <= 1e-14


@pytest.mark.parametrize("name", ["mixed", "s64", "default"])
def test_view_rays_at_the_reference_pose_has_the_reference_orientation(name):
    """At the pose of the scene's own camera — looking along +z, its fov over the screen's width, a frame
    of the screen's aspect — the reference's directions to 1e-15 per component: the orientation.  (For
    these cameras, whose screen width is a power of two, view_rays' order of operations gives the
    reference's very bits, which is what lets render_view meet the rendered frame; that is checked on the
    GPU, where it matters.)"""
    cam = Q.elems_of(name)[0].u.camera
    w = 64
    h = int(round(w * cam.screen_height / cam.screen_width))
    assert h * cam.screen_width == w * cam.screen_height
    loc, ref = Q.camera_rays(name, w, h)
    e, d = raytracer.view_rays(w, h, tuple(loc), tuple(loc + np.array([0.0, 0.0, 1.0])), fov=cam.fov)
    assert np.array_equal(e, loc) and np.abs(d - ref).max() <= 1e-15


@pytest.mark.parametrize("kw", [
    dict(eye=(1, 2, 3), target=(1, 2, 3)), dict(eye=(0, 0, 0), target=(0, 5, 0)), dict(eye=(0, 0, 0), target=(0, -1, 0)),
    dict(eye=(0, 0, 0), target=(0, 0, 1), up=(0, 0, 0)), dict(eye=(0, 0, 0), target=(0, 0, 1), up=(0, 0, -3)),
    dict(eye=(0, 0, 0), target=(0, 0, 1), fov=0), dict(eye=(0, 0, 0), target=(0, 0, 1), fov=180),
    dict(eye=(0, 0, 0), target=(0, 0, 1), fov=-5), dict(eye=(0, 0, 0), target=(0, 0, 1), fov="wide"),
    dict(eye=(0, 0), target=(0, 0, 1)), dict(eye=(0, 0, 0), target=(0, 0, float("nan"))), dict(eye="here", target=(0, 0, 1))])
def test_view_rays_refuses(kw):
    with pytest.raises(ValueError):
        raytracer.view_rays(4, 3, **kw)
    with pytest.raises(ValueError):
        raytracer.view_rays(0, 3, (0, 0, 0), (0, 0, 1))


# ---- trace_rays' own checks ----------------------------------------------------------------------
def boom():
    raise AssertionError("the library was loaded")


O3, D3 = np.zeros(3), np.ones((5, 3))


@pytest.mark.parametrize("args,kw", [
    ((O3, np.ones(3), 3), {}), ((O3, np.ones((5, 2)), 3), {}), ((np.zeros((4, 3)), D3, 3), {}), ((np.zeros(2), D3, 3), {}),
    ((O3, np.ones((5, 3), dtype=bool), 3), {}), ((O3, [[1, 2, None]], 3), {}), ((O3, D3, -1), {}), ((O3, D3, 2.0), {}),
    ((O3, D3, True), {}), ((O3, D3, 1 << 32), {}), ((O3, D3, 3), dict(precision="u8")), ((O3, D3, 3), dict(precision="f16")),
    ((O3, D3, 3), dict(levels=1)), ((O3, D3, 3), dict(device=-1)), ((O3, D3, 3), dict(device=True))])
def test_trace_rays_refuses_bad_arguments_without_the_library(monkeypatch, args, kw):
    monkeypatch.setattr(N, "lib", boom)
    with pytest.raises(ValueError):
        raytracer.trace_rays(*args, records.scene(), **kw)


def test_trace_rays_checks_scenes_and_empty_batches_without_the_library(monkeypatch):
    monkeypatch.setattr(N, "lib", boom)
    with pytest.raises(ValueError):  # a scene marshal refuses
        raytracer.trace_rays(O3, D3, 3, records.scene()[1:])
    got = raytracer.trace_rays(O3, np.zeros((0, 3)), 3, records.scene(), precision="f32")
    assert got.shape == (0, 3) and got.dtype == np.float32
    rgb, lv = raytracer.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)), 0, levels=True)
    assert rgb.shape == (0, 3) and rgb.dtype == np.float64 and lv.shape == (0,) and lv.dtype == np.uint8
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.trace_rays([0, 0, -2], [[0, 0, 1], [1, 0, 0]], 2, records.scene(), precision="f32", levels=True)
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.render_view(4, 3, 2, records.scene(), eye=(0, 0, -2), target=(0, 0, 10))
    with pytest.raises(ValueError):
        raytracer.render_view(4, 3, 2, records.scene(), eye=(0, 0, -2), target=(0, 0, -2))


# ---- the population of the GPU tests' subsets, on the reference alone -----------------------------
def differ(a, b):
    return (a != b).any(axis=1)


@pytest.mark.parametrize("name", T.INCOHERENT)
def test_restatement_subsets_hold_what_they_are_chosen_for(name):
    depth = T.INCOHERENT_DEPTH
    idx, rgb, lv = T.incoherent_ref(name)
    assert len(idx) >= T.N_SUBSET and len(idx) % 64 and len(set(idx.tolist())) == len(idx)
    assert np.isfinite(rgb).all() and (rgb >= 0).all()
    counts = np.bincount(lv, minlength=depth + 1)
    print(name, "chain lengths", counts.tolist(), flush=True)
    assert counts[0] >= 20, "misses"
    assert (rgb[lv == 0] == 0).all() and (rgb[lv > 0] != 0).any()
    for k in range(1, min(depth, 3) + 1):
        assert counts[k] >= 5, f"chains of length {k}"
    assert differ(rgb, T.incoherent_unshadowed(name)).sum() >= 20, "shadows change too few colours"
    assert differ(rgb, T.incoherent_depth1(name)).sum() >= 20, "reflections change too few colours"
    if name == "s2+ties":
        ties = Q.incoherent("s2+ties")[2]["ties"]
        assert ties[idx].sum() >= 1, "no ray of the subset has an exact tie"
    assert T.unit_powers(name) == (name in ("s64~u", "s2+ties"))


def test_variant_scenes():
    assert T.unit_powers("s64~u") and not T.unit_powers("s64") and not T.unit_powers("default")
    assert T.n_lights("default~1") == 1 and T.n_lights("s64~dark") == 0 and T.n_lights("s20l33") > 32
    assert len(T.scene_of("default~1")) == len(T.scene_of("default")) - T.n_lights("default") + 1
    # a chain in a scene without lights stops after one object; the colour is zero
    o, d, _, _ = Q.incoherent("s64")
    rgb, lv = T.restate(T.scene_of("s64~dark"), o, d, 4, np.arange(0, 400))
    assert lv.max() == 1 and (lv == 0).any() and not rgb.any()

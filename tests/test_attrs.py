"""Primary-hit attributes (RT_ATTRIBUTES in include/rt_mi355x.h) on the CPU: the header's
declaration, the ctypes layout of rt_attr_planes, rt_launch_attrs' argument checks (all made before
any HIP call and before the context is read, so no device is needed), the checks of
raytracer.render_attributes and raytracer.pick (made before the library is loaded), the reference
tests/attr_ref.py the GPU tests compare against (its frames hold what they are chosen for, and its
restatement of the jitter is the oracle's), and the scene compiler's table from compact object id
to scene-list index under the host sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer, records, scenes
from tests import attr_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
W, H = 200, 150
WIN = (37, 21, 83, 59)
FIELDS = ("struct_size", "precision", "d_elem", "d_t", "d_point", "d_normal", "d_albedo")
# (scene, width, height) of the reference frames, and what each holds:
# (misses, sphere hits, triangle hits, plane hits, distinct objects hit), None = not pinned
FRAMES = {
    ("mixed", 128, 96): (2113, 2698, 966, 6511, 39),
    ("default", 64, 48): (1153, 1122, 149, 648, None),
    ("s2+ties", 64, 48): (None, 147, None, None, None),
    ("mixed_int@inside_cloud", 64, 48): (None, None, None, None, None),
    ("s64", 96, 96): (6639, 2577, None, None, None),
}


def test_header_declares_rt_launch_attrs():
    src = open(HEADER).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    m = re.search(r"\bint rt_launch_attrs\(([^;]*)\);", src)
    assert m, "the header does not declare rt_launch_attrs"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "p", "width", "height", "x0", "y0", "win_w", "win_h", "row_block", "shard", "nshards", "spp", "seed", "sample",
        "planes", "stream"]
    assert "rt_launch_attrs" in N.EXPORTS and not any(ch.isdigit() for ch in "rt_launch_attrs")
    assert "RT_ATTRIBUTES" in src
    body = re.search(r"typedef struct rt_attr_planes \{(.*?)\} rt_attr_planes;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()] == list(FIELDS)


def test_attr_planes_layout_matches_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_mi355x.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_attr_planes), offsetof(rt_attr_planes, struct_size),
 offsetof(rt_attr_planes, precision), offsetof(rt_attr_planes, d_elem), offsetof(rt_attr_planes, d_t),
 offsetof(rt_attr_planes, d_point), offsetof(rt_attr_planes, d_normal), offsetof(rt_attr_planes, d_albedo)); return 0;}
'''
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [ctypes.sizeof(N.RtAttrPlanes)] + [getattr(N.RtAttrPlanes, f).offset for f in FIELDS]
    assert [f for f, _ in N.RtAttrPlanes._fields_] == list(FIELDS)


A8 = 0x10000  # a pointer never dereferenced, aligned for every plane


def planes(precision=N.RT_OUT_F64, elem=A8, t=A8, point=A8, normal=A8, albedo=A8, struct_size=None):
    size = ctypes.sizeof(N.RtAttrPlanes) if struct_size is None else struct_size
    return N.RtAttrPlanes(size, precision, elem, t, point, normal, albedo)


def call(L, pl, *, p=A8, w=W, h=H, win=WIN, rb=16, shard=0, nshards=1, spp=1, seed=0, sample=0):
    return L.rt_launch_attrs(p, w, h, *win, rb, shard, nshards, spp, seed, sample,
                             ctypes.byref(pl) if pl is not None else None, None)


def test_argument_checks_need_no_device_and_never_read_the_context(native):
    """Every documented argument error, with a context pointer that is null or would fault if read."""
    L = native.lib()
    bad, big = N.RT_EBADARG, N.RT_ETOOBIG
    assert call(L, planes(), p=None) == bad
    assert call(L, None) == bad
    last = N.RtAttrPlanes.d_albedo.offset
    for size in (0, 8, last, last + 7):  # ends before d_albedo, or inside it
        assert call(L, planes(struct_size=size)) == bad, size
    assert call(L, planes(elem=None, t=None, point=None, normal=None, albedo=None)) == bad
    for prec in (N.RT_OUT_U8, N.RT_OUT_U16, -1, 4):
        assert call(L, planes(precision=prec)) == bad, prec
    assert call(L, planes(), spp=0) == bad
    assert call(L, planes(), spp=3, sample=3) == bad
    assert call(L, planes(), spp=1, sample=1) == bad
    assert call(L, planes(), spp=N.RT_MAX_SPP, sample=N.RT_MAX_SPP) == bad
    assert call(L, planes(), spp=N.RT_MAX_SPP + 1, sample=0) == big
    # alignment: d_elem to 4 bytes, a float plane to its element
    assert call(L, planes(elem=A8 + 2)) == bad
    for name in ("t", "point", "normal", "albedo"):
        assert call(L, planes(**{name: A8 + 4})) == bad, name                       # f64: 8 bytes
        assert call(L, planes(N.RT_OUT_F32, **{name: A8 + 2})) == bad, name         # f32: 4 bytes
    # the window, shard and size errors of rt_launch_window
    for win in ((0, 0, 0, 10), (0, 0, 10, 0), (5, 0, 0, 0), (150, 0, 51, 10), (0, 100, 10, 51), (200, 0, 1, 1),
                (0xFFFFFFF0, 0, 0x20, 1)):
        assert call(L, planes(), win=win) == bad, win
    assert call(L, planes(), rb=0) == bad
    assert call(L, planes(), nshards=0) == bad
    assert call(L, planes(), shard=1, nshards=1) == bad
    assert call(L, planes(), w=0) == bad and call(L, planes(), h=0) == bad
    assert call(L, planes(), w=(1 << 20) + 1) == big and call(L, planes(), h=(1 << 20) + 1) == big


def test_valid_arguments_reach_the_null_context(native):
    """Valid arguments of every kind — a window, the whole frame, one plane, binary32, a shard, a
    sample of a supersampled frame, a struct that ends right after d_albedo — get as far as the
    null context (on any machine: the context is only read once everything else is accepted)."""
    L = native.lib()
    ok = dict(p=None)
    assert call(L, planes(), **ok) == N.RT_EBADARG
    assert call(L, planes(), win=(0, 0, W, H), **ok) == N.RT_EBADARG
    assert call(L, planes(t=None, point=None, normal=None, albedo=None), **ok) == N.RT_EBADARG
    assert call(L, planes(N.RT_OUT_F32, t=A8 + 4, point=A8 + 4), **ok) == N.RT_EBADARG
    assert call(L, planes(), rb=7, shard=2, nshards=3, spp=3, seed=(1 << 64) - 1, sample=2, **ok) == N.RT_EBADARG


def boom():
    raise AssertionError("the library was loaded")


@pytest.mark.parametrize("kw", [
    dict(window=(0, 0, 0, 10)), dict(window=(150, 0, 51, 10)), dict(window=(0, 100, 10, 51)), dict(window=(-1, 0, 10, 10)),
    dict(window=(0, 0, 10)), dict(window=(0, 0, 10.0, 10)), dict(window="abcd"), dict(window=(0, 0, True, 1)),
    dict(planes=()), dict(planes=("elem", "depth")), dict(planes="elem"), dict(planes=("t", "t")), dict(planes=(1,)),
    dict(precision="u8"), dict(precision="f16"),
    dict(spp=0), dict(spp=N.RT_MAX_SPP + 1), dict(spp=3, sample=3), dict(sample=1), dict(sample=-1), dict(spp=2.0),
    dict(spp=True), dict(seed=-1), dict(seed=1 << 64), dict(device=-1)])
def test_render_attributes_refuses_bad_arguments_without_the_library(monkeypatch, kw):
    monkeypatch.setattr(N, "lib", boom)
    with pytest.raises(ValueError):
        raytracer.render_attributes(W, H, records.scene(), **kw)


def test_render_attributes_and_pick_check_sizes_pixels_and_scenes_without_the_library(monkeypatch):
    monkeypatch.setattr(N, "lib", boom)
    for w, h in ((0, 0), (0, 5), (5, 0), (-1, 5), (5.0, 5), (True, 5)):
        with pytest.raises(ValueError):
            raytracer.render_attributes(w, h, records.scene())
        with pytest.raises(ValueError):
            raytracer.pick(w, h, 0, 0, records.scene())
    for x, y in ((W, 0), (0, H), (-1, 0), (0, -1), (1.0, 1), (True, 1), (None, 0)):
        with pytest.raises(ValueError):
            raytracer.pick(W, H, x, y, records.scene())
    with pytest.raises(ValueError):  # a scene marshal refuses
        raytracer.render_attributes(W, H, records.scene()[1:])
    # good arguments pass the checks and reach the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.render_attributes(W, H, records.scene(), window=WIN, planes=("t", "normal"), precision="f32", spp=3,
                                    seed=7, sample=2)
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.pick(W, H, W - 1, H - 1, records.scene())


@pytest.mark.parametrize("name,w,h", sorted(FRAMES))
def test_reference_frames_hold_what_they_are_chosen_for(name, w, h):
    """The figures measured when the tests were written, so a changed scene generator fails loudly;
    and no float of a reference is non-finite (d_t at a miss aside: the contract's +inf), a negative
    zero, or non-zero below 2^-126 — so a binary32 plane is exactly astype(float32) of the binary64
    one, and no value needs to be left out of a comparison."""
    ref = A.frame(name, w, h, ties=(name == "s2+ties"))
    got = A.kinds(name, ref)
    print(name, w, h, "misses, sphere, triangle, plane hits, distinct objects:", got, flush=True)
    for g, want in zip(got, FRAMES[(name, w, h)]):
        assert want is None or g == want, (name, got, FRAMES[(name, w, h)])
    hit = ref["elem"] >= 0
    assert got[0] > 0 and hit.any()
    if name == "s2+ties":
        n = int((ref["ties"] & hit).sum())
        print("hits with a second object at exactly the same t:", n, flush=True)
        assert n == 59
    if name == "mixed_int@inside_cloud":
        n = int((ref["t"][hit] < 0).sum())
        print("hits with t < 0:", n, flush=True)
        assert n == 266
    assert np.all(ref["elem"][hit] >= 1) and np.all(ref["elem"][~hit] == -1)
    assert np.all(np.isposinf(ref["t"][~hit])) and np.all(np.isfinite(ref["t"][hit]))
    for k in ("t", "point", "normal", "albedo"):
        a = ref[k]
        vals = a[hit]
        assert np.all(np.isfinite(vals)), k
        assert not np.any((a == 0) & np.signbit(a)), (k, "a negative zero")
        assert not np.any((a != 0) & (np.abs(a) < 2.0 ** -126)), (k, "a value below the binary32 normal range")
        assert np.all(np.isfinite(vals.astype(np.float32))), (k, "overflows binary32")
        if k != "t":
            assert not np.any(a[~hit]), (k, "a miss that is not all zero")


def test_jitter_restatement_is_the_oracles(oracle):
    """attr_ref.sample_xy against the oracle's own supersampling: the 3-sample pixel is
    (c0 + c1 + c2) / 3 of the traces at the restated positions, bit for bit."""
    w = h = 16
    depth, seed = 5, 0x5EED0003
    el = N.marshal(scenes.named("s64"))
    img = oracle.render(el, w, h, depth, mode=oracle.MEMO, spp=3, seed=seed)
    one = oracle.render(el, w, h, depth, mode=oracle.MEMO)
    hits = 0
    for x, y in ((0, 0), (7, 8), (8, 7), (15, 15), (3, 12), (12, 3), (5, 5), (10, 9), (6, 10)):
        c = [np.array(oracle.trace_pixel(el, *A.sample_xy(x, y, w, h, 3, seed, s), depth, mode=oracle.MEMO)[0])
             for s in range(3)]
        want = (c[0] + c[1] + c[2]) / 3.0
        assert want.tobytes() == img[y, x].tobytes(), (x, y, want, img[y, x])
        hits += bool(want.any())
    assert hits >= 3, "the pixels chosen are nearly all background"
    assert img.tobytes() != one.tobytes()
    # spp = 1 is the reference's position
    assert A.sample_xy(5, 7, w, h) == (5 / w, 7 / h)


def test_elem_table_under_host_sanitizers(tmp_path):
    """Compiled::elem_of (rt_scene.cpp), the table behind d_elem, built with AddressSanitizer + UBSan
    in a stand-alone program: strictly increasing, only sphere, triangle and plane elements, all of
    them — on the mixed scene and on a scene with terms of no known kind between its objects."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "elem_table_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "csrc", "elem_table_check.cpp"),
                    os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_scene.cpp"), "-o", exe], check=True)
    base = records.scene()
    other = [base[0], ("mesh", 1, 2)]
    for t in base[1:]:
        other += [t, ("mesh", len(other)), "a string"]
    want, files = [], []
    for i, sc in enumerate((scenes.named("mixed"), other, records.scene())):
        el = N.marshal(sc)
        objs = [j for j in range(len(el)) if el[j].kind in (N.RT_SPHERE, N.RT_TRIANGLE, N.RT_PLANE)]
        want.append([len(el), len(objs)] + objs)
        path = tmp_path / f"s{i}.bin"
        path.write_bytes(bytes(el))
        files.append(str(path))
    assert sum(e.kind == N.RT_OTHER for e in N.marshal(other)) >= 10
    assert want[1][2:] != want[2][2:] and want[1][1] == want[2][1]  # the same objects at other positions
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [list(map(int, ln.split())) for ln in r.stdout.splitlines()] == want

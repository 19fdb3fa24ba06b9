"""The hostile scenes (tests/hostile.py) on the CPU: none of them is vacuous.

* the scene compiler's flags per scene, against a table that holds every flag in both states
  (so each filter branch the scenes are meant for is really compiled in);
* the oracle's frame of every scene is finite, has hits and reflections (or, for the dz = 0
  camera, none), and shows the one property each construction is for;
* the ties and the zero direction vector are the reference's own behaviour: the C oracle equals
  the term-level restatement (oracle/erl_restatement.py) bit for bit.

The stand-alone ASan + UBSan run of the scene compiler on these scenes is
tests/test_host.py::test_scene_compiler_under_host_sanitizers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import terms
from tests import hostile as H
from tests.test_oracle import _bits, _py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HGT = 64, 48

# cull_ok beam_ok occ_ok occ_cells bvh_ok bvh_depth norm_ok prim_ok staged (l_bytes > 0), from the
# thresholds of rt_layout.h: beams from 8 spheres, 16 cells and the BVH from 128 spheres, occluder
# masks up to 2^24 (light, target, sphere) tests, LDS staging for spheres-only scenes up to 32 KiB,
# BVH depth <= ceil(log2 n) + 2, everything off beyond CULL_EXTENT.
SMALL = (1, 1, 1, 1, 0, 0, 1, 1, 1)      # spheres only, staged, one cell, no BVH
MIXED = (1, 1, 1, 1, 0, 0, 0, 1, 0)      # triangles and planes: no staging, no norm_ok
FLAGS = {
    "s7+g": SMALL, "s8+g": SMALL, "s16+g": SMALL, "s7+g_swapped": SMALL,
    "s7+d": (1, 1, 1, 1, 0, 0, 0, 1, 1), "s8+d": (1, 1, 1, 1, 0, 0, 0, 1, 1), "s16+d": (1, 1, 1, 1, 0, 0, 0, 1, 1),
    "s2+ties": (1, 0, 1, 1, 0, 0, 1, 1, 1),
    "s160+g": (1, 1, 1, 16, 1, 10, 1, 1, 0), "s160+d": (1, 1, 1, 16, 1, 10, 0, 1, 0),
    "mixed_int+g": MIXED, "mixed_int+d": MIXED,
    "s300l190+g": (1, 1, 0, 16, 1, 11, 1, 1, 0), "s300l190+d": (1, 1, 0, 16, 1, 11, 0, 1, 0),
    "lattice": (1, 1, 1, 16, 1, 10, 1, 1, 0),
    "far4900": SMALL, "far5100": SMALL, "far9970": SMALL,
    "far10100": (0, 0, 0, 1, 0, 0, 0, 1, 0),
}
for _c in H.CAMERAS:
    _p = 0 if _c in ("tiny_origin", "dz0") else 1
    FLAGS[f"s64@{_c}"] = SMALL[:7] + (_p,) + SMALL[8:]
    FLAGS[f"mixed_int@{_c}"] = MIXED[:7] + (_p,) + MIXED[8:]
FLAG_NAMES = ("cull_ok", "beam_ok", "occ_ok", "occ_cells", "bvh_ok", "bvh_depth", "norm_ok", "prim_ok", "staged")
# ext to the nearest unit, where the scene is about the extent
EXT = {"far4900": 4912, "far5100": 5112, "far9970": 9982, "far10100": 10112}


def _ext(scene):
    """SceneHdr::ext restated: the largest |coordinate| of the origins and sphere centres, and |radius|."""
    m = 0.0
    for t in scene:
        if t[0] == "camera":
            m = max([m] + [abs(float(v)) for v in t[1][1:]])
        elif t[0] == "point_light":
            m = max([m] + [abs(float(v)) for v in t[2][1:]])
        elif t[0] == "sphere":
            m = max([m, abs(float(t[1]))] + [abs(float(v)) for v in t[2][1:]])
    return m


def test_scenes_are_deterministic_and_exact_in_text():
    assert set(FLAGS) == set(H.NAMES)
    for name in H.NAMES:
        sc = H.build(name)
        assert terms.exact_eq(sc, H.build(name)), name
        assert terms.exact_eq(terms.parse_term(terms.format_term(sc) + "."), sc), name
        for t in sc:
            if t[0] in ("sphere", "triangle", "plane"):
                m = t[-1]
                assert m[2] in (0, 1), (name, m)
                assert all(0 <= c <= 1 for c in m[1][1:]), (name, m)
    assert sum(t[0] == "sphere" for t in H.build("lattice")) == 175


def test_compiled_flags_table(tmp_path):
    """Every hostile scene compiles to the flags its construction is meant to give, and the table
    holds every flag in both states and ext on both sides of 5000 and of CULL_EXTENT."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "scene_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "csrc", "scene_check.cpp"),
                    os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_scene.cpp"), "-o", exe], check=True)
    files = []
    for i, name in enumerate(H.NAMES):
        p = tmp_path / f"h{i}.bin"
        p.write_bytes(bytes(N.marshal(H.build(name))))
        files.append(str(p))
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}  # the thresholds' defaults
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(H.NAMES)
    seen = {f: set() for f in FLAG_NAMES}
    exts = []
    for name, row in zip(H.NAMES, rows):
        assert row[:3] == ["0", "0", "0"], (name, row)
        got = tuple(int(v) for v in row[5:14])
        assert got == FLAGS[name], (name, dict(zip(FLAG_NAMES, got)))
        ext = float(row[14])
        assert ext == _ext(H.build(name)), name
        if name in EXT:
            assert abs(ext - EXT[name]) < 0.5, (name, ext)
        exts.append(ext)
        for f, v in zip(FLAG_NAMES, got):
            seen[f].add(v)
    for f in FLAG_NAMES:
        if f == "occ_cells":
            assert seen[f] == {1, 16}
        elif f == "bvh_depth":
            assert 0 in seen[f] and max(seen[f]) > 0
        else:
            assert seen[f] == {0, 1}, f
    assert any(e < 5000 for e in exts) and any(5000 < e <= 1e4 for e in exts) and any(e > 1e4 for e in exts)
    # both sides of the spheres-only binary32 beams' bound (make_beam32: 2 ext (1 + 1e-6) <=
    # CULL_EXTENT (1 - 1e-6)), and within 0.2 % of CULL_EXTENT from inside
    assert any(2 * e <= 1e4 and e > 4000 for e in exts) and any(1e4 < 2 * e and e <= 1e4 for e in exts)
    assert any(1e4 * (1 - 2e-3) < e <= 1e4 for e in exts)


@pytest.mark.parametrize("name", H.NAMES)
def test_oracle_frames_are_not_vacuous(oracle, name):
    """Finite, at least 50 hit pixels and a chain of at least 2 levels; the dz = 0 camera over S64
    (every ray in the plane z = -2, every sphere beyond z = 4) hits nothing at all."""
    img, lv = H.oracle_ref(oracle, name, W, HGT)
    assert np.all(np.isfinite(img))
    if name == "s64@dz0":
        assert int((lv > 0).sum()) == 0 and not img.any()
        return
    assert int((lv > 0).sum()) >= 50, int((lv > 0).sum())
    assert int(lv.max()) >= 2


def test_swapped_pair_differs_in_the_centre_column_only(oracle):
    """The mirrored pair is hit at equal distance by the rays with x = 0 (column W/2): the earlier of
    the two in the list wins there, and nowhere else does the order matter."""
    a, _ = H.oracle_ref(oracle, "s7+g", W, HGT)
    b, _ = H.oracle_ref(oracle, "s7+g_swapped", W, HGT)
    diff = ~np.all(_bits(a) == _bits(b), axis=-1)
    assert diff.any()
    assert not np.delete(diff, W // 2, axis=1).any(), np.argwhere(diff).tolist()


def test_lattice_centre_pixel_reaches_full_depth(oracle):
    _, lv = H.oracle_ref(oracle, "lattice", W, HGT)
    assert int(lv[HGT // 2, W // 2]) == H.depth("lattice") == 8


def test_far_scenes_keep_the_chains_of_s64(oracle):
    """Moving everything by (4900..10100, ...) keeps the levels histogram of the unshifted scene."""
    el = N.marshal(H.base("s64"))
    _, lv0 = oracle.render(el, W, HGT, 5, mode=oracle.MEMO, levels=True)
    h0 = np.bincount(lv0.ravel(), minlength=6)
    for name in H.FAR_SHIFTS:
        _, lv = H.oracle_ref(oracle, name, W, HGT)
        assert np.array_equal(np.bincount(lv.ravel(), minlength=6), h0), name


@pytest.mark.parametrize("name", ["s7+g", "s7+d", "s64@dz0", "mixed_int@dz0", "s64@negscreen", "mixed_int@negscreen"])
def test_c_oracle_equals_term_restatement_on_hostile_scenes(oracle, name):
    """Ties (twins, 2 vs 2.0, the mirrored pair), degenerate spheres, lights on and in spheres, the
    zero direction vector and the negative focal length: the C oracle gives the term-level
    restatement's bits at 24x18, so these behaviours are the reference's own."""
    scene = H.build(name)
    el = N.marshal(scene)
    for d in (1, 3):
        a = oracle.render(el, 24, 18, d, mode=oracle.MEMO)
        b = _py(scene, 24, 18, d)
        assert np.array_equal(_bits(a), _bits(b)), f"{name} depth {d}"

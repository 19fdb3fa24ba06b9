"""The flat hostile scenes (tests/hostile_flat.py) on the CPU: none of them is vacuous.

* the scene compiler's flags and object counts per scene, against a table in which a scene without
  spheres occurs and beam_ok and bvh_ok occur in both states;
* per scene, from the oracle at 64x48: the frame is finite and shows the property the construction
  is for (counts of plane and triangle primaries, chain lengths, ties, negative and huge distances);
  every count is printed;
* the ties across kinds, the zero normal, the negative distances and the non-unit normals are the
  reference's own behaviour: the C oracle equals the term-level restatement
  (oracle/erl_restatement.py) bit for bit.

The thresholds are lower bounds under the counts the oracle gives (in the comments), never
tolerances.  The stand-alone ASan + UBSan run of the scene compiler on these scenes is
tests/test_host.py::test_scene_compiler_under_host_sanitizers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import terms
from tests import attr_ref as A
from tests import hostile_flat as F
from tests.test_oracle import _bits, _py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HGT = 64, 48
CX, CY = W // 2, HGT // 2  # X = Y = 0.5: the ray (0, 0, 1) exactly

# cull_ok beam_ok occ_ok occ_cells bvh_ok bvh_depth norm_ok prim_ok staged, then n_sph n_tri n_pl.
# Beams from 8 spheres and occluder masks from one; no LDS staging and no norm_ok with a flat object.
FLAG_NAMES = ("cull_ok", "beam_ok", "occ_ok", "occ_cells", "bvh_ok", "bvh_depth", "norm_ok", "prim_ok", "staged")
NINE = (1, 1, 1, 1, 0, 0, 0, 1, 0)       # sph9 (or ten spheres) and flat objects
NO_SPH = (1, 0, 0, 1, 0, 0, 0, 1, 0)     # no sphere: no beams, no occluder masks
FLAGS = {
    "corridor": NINE + (9, 0, 3), "corridor_nonunit": NINE + (9, 0, 3), "mirror_nonunit": NINE + (9, 0, 2),
    "planes_only": NO_SPH + (0, 0, 3), "tris_only": NO_SPH + (0, 96, 0),
    "empty": (1, 0, 0, 1, 0, 0, 1, 1, 0) + (0, 0, 0),
    "tie3_tps": NINE + (10, 1, 1), "tie3_pst": NINE + (10, 1, 1), "tie3_stp": NINE + (10, 1, 1),
    "mesh": NINE + (9, 96, 0), "mesh_small": NINE + (9, 8, 0),
    "behind_facing": NINE + (9, 1, 1), "behind_away": NINE + (9, 1, 1),
    "zero_normal": NINE + (9, 1, 0),
    "graze12": NINE + (9, 0, 2), "graze16": NINE + (9, 0, 2),
    "pencil_wall": NINE + (10, 0, 1), "pencil_fartri": NINE + (10, 1, 0),
    "big_flat": (1, 1, 1, 16, 1, 10, 0, 1, 0) + (160, 8, 3),
}


def test_scenes_are_deterministic_and_exact_in_text():
    assert set(FLAGS) == set(F.NAMES)
    for name in F.NAMES:
        sc = F.build(name)
        assert terms.exact_eq(sc, F.build(name)), name
        assert terms.exact_eq(terms.parse_term(terms.format_term(sc) + "."), sc), name
        powers = []
        for t in sc:
            if t[0] in ("sphere", "triangle", "plane"):
                m = t[-1]
                powers.append(m[2])
                assert all(0 <= c <= 1 for c in m[1][1:]), (name, m)
            if t[0] == "plane":
                mag2 = sum(float(c) ** 2 for c in t[1][1:])
                assert 0.25 <= mag2 <= 4, (name, t)
        assert powers == [i % 2 for i in range(len(powers))], name
    assert len(F.build("mesh")) - len(F.build("tris_only")) == 9 and len(F.build("mesh")) == 3 + 105


def test_compiled_flags_table(tmp_path):
    """Every flat hostile scene compiles to the flags and counts its construction is meant to give."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "scene_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "csrc", "scene_check.cpp"),
                    os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_scene.cpp"), "-o", exe], check=True)
    files = []
    for i, name in enumerate(F.NAMES):
        p = tmp_path / f"f{i}.bin"
        p.write_bytes(bytes(N.marshal(F.build(name))))
        files.append(str(p))
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}  # the thresholds' defaults
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(F.NAMES)
    seen = {f: set() for f in FLAG_NAMES + ("n_sph",)}
    for name, row in zip(F.NAMES, rows):
        assert row[:3] == ["0", "0", "0"], (name, row)
        got = tuple(int(v) for v in row[5:14]) + tuple(int(v) for v in row[15:18])
        print(name, dict(zip(FLAG_NAMES + ("n_sph", "n_tri", "n_pl"), got)), "ext", row[14], "n_chunk", row[18], flush=True)
        assert got == FLAGS[name], (name, dict(zip(FLAG_NAMES + ("n_sph", "n_tri", "n_pl"), got)))
        n_sph, n_tri, n_pl = got[9:]
        assert int(row[18]) == (n_sph + 63) // 64, (name, row)
        if n_tri or n_pl:
            assert got[FLAG_NAMES.index("norm_ok")] == 0, name
        # ext bounds the origins and the spheres only: every scene here compiles with culling on,
        # however far its flat objects reach
        assert got[0] == 1 and float(row[14]) <= 40, (name, row[14])
        for f, v in zip(FLAG_NAMES + ("n_sph",), got[:10]):
            seen[f].add(v)
    assert 0 in seen["n_sph"] and max(seen["n_sph"]) > 128
    assert seen["beam_ok"] == {0, 1} and seen["bvh_ok"] == {0, 1} and seen["occ_ok"] == {0, 1}


def _frames(oracle, name):
    img, lv = F.oracle_ref(oracle, name, W, HGT)
    assert np.all(np.isfinite(img)), name
    ref = A.frame(name, W, HGT, ties=True)
    _miss, n_s, n_t, n_p, _ = A.kinds(name, ref)
    hist = np.bincount(lv.ravel(), minlength=F.depth(name) + 1).tolist()
    hit = ref["elem"] >= 0
    t = ref["t"][hit]
    print(f"{name}: primaries sphere {n_s} triangle {n_t} plane {n_p}; levels {hist}; ties {int(ref['ties'].sum())}; "
          f"t in [{t.min() if t.size else None}, {t.max() if t.size else None}]; max channel {img.max():.4g}", flush=True)
    return img, lv, ref, (n_s, n_t, n_p), t


@pytest.mark.parametrize("name", ["corridor", "planes_only"])
def test_corridor_chains_reach_the_depth_limit(oracle, name):
    """Measured: 2936 (planes_only 3072) plane primaries, 3008 pixels at level 8."""
    _, lv, _, (n_s, _n_t, n_p), _ = _frames(oracle, name)
    assert n_p >= 2500 and int((lv == 8).sum()) >= 2500
    assert (n_s == 0) == (name == "planes_only")


def test_corridor_nonunit_differs_from_unit_normals(oracle):
    """Measured: levels 1 to 5 on 57 / 1509 / 1456 / 47 / 3 pixels.  The two writings of a plane are
    the same point set and different normals: the frames differ."""
    img, lv, _, _, _ = _frames(oracle, "corridor_nonunit")
    assert int(lv.max()) >= 4
    unit = oracle.render(N.marshal(F.build("corridor")), W, HGT, F.depth("corridor_nonunit"), mode=oracle.MEMO)
    n = int((~np.all(_bits(img) == _bits(unit), axis=-1)).sum())
    print("corridor_nonunit: pixels that differ from corridor at depth 6:", n, flush=True)
    assert n >= 1000  # measured: 3008


def _nonunit_rays(oracle, name, w, h):
    """The reflection chains of the frame restated ray by ray (oracle.nearest and the reference's
    bounce): (rays whose |d|^2 is outside 1 +- 1e-6 that hit something, those that hit a sphere)."""
    el = N.marshal(F.build(name))
    cam = el[0]
    loc = (cam.u.camera.location.x, cam.u.camera.location.y, cam.u.camera.location.z)
    n_any = n_sph = 0
    for y in range(h):
        for x in range(w):
            o, d = loc, oracle.shoot_ray(loc, oracle.point_on_screen(cam, x / w, y / h))
            for _ in range(F.depth(name)):
                hit = oracle.nearest(el, o, d)
                if hit is None:
                    break
                i, _t, o, n = hit
                if abs(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - 1) > 1e-6:
                    n_any += 1
                    n_sph += el[i].kind == N.RT_SPHERE
                d = oracle.vec_op("bounce", d, n)
    return n_any, n_sph


@pytest.mark.parametrize("name,min_any,min_sph", [("corridor_nonunit", 3000, 10), ("mirror_nonunit", 1500, 250)])
def test_nonunit_reflections_hit_spheres(oracle, name, min_any, min_sph):
    """Measured at 64x48: corridor_nonunit 4077 rays that are not unit vectors hit something, 13 of
    them a sphere; mirror_nonunit 1763 and 271 (at 320x240 45,256 and 6694).  A sphere scan that
    mistook such a ray for a unit vector would lose those hits."""
    _frames(oracle, name)
    n_any, n_sph = _nonunit_rays(oracle, name, W, HGT)
    print(f"{name}: rays with |d|^2 outside 1 +- 1e-6 that hit: {n_any}, a sphere: {n_sph}", flush=True)
    assert n_any >= min_any and n_sph >= min_sph


@pytest.mark.parametrize("order", ["tps", "pst", "stp"])
def test_tie3_first_listed_wins(oracle, order):
    name = f"tie3_{order}"
    _, _, ref, _, _ = _frames(oracle, name)
    el = N.marshal(F.build(name))
    kinds = {"t": N.RT_TRIANGLE, "p": N.RT_PLANE, "s": N.RT_SPHERE}
    assert [el[3 + i].kind for i in range(3)] == [kinds[k] for k in order]
    hits = [oracle.intersect(el[3 + i], (0, 0, -2), (0, 0, 1)) for i in range(3)]
    assert all(h is not None and h[0] == 12.0 for h in hits), hits
    assert int(ref["elem"][CY, CX]) == 3 and ref["t"][CY, CX] == 12.0 and bool(ref["ties"][CY, CX])


def test_tie3_frames_differ_pairwise(oracle):
    f = [F.oracle_ref(oracle, f"tie3_{o}", W, HGT)[0] for o in ("tps", "pst", "stp")]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(_bits(f[a]), _bits(f[b]))


@pytest.mark.parametrize("name", ["mesh", "tris_only"])
def test_mesh_has_shared_edge_ties(oracle, name):
    """Measured: 821 triangle primaries, 105 pixels where a second triangle is hit at exactly the
    nearest one's t (shared edges and corners), 820 chains at level 5."""
    _, lv, ref, (n_s, n_t, _n_p), _ = _frames(oracle, name)
    assert n_t >= 800 and int(ref["ties"].sum()) >= 100
    assert int((lv == 5).sum()) >= 800
    if name == "tris_only":
        assert n_s == 0


def test_behind_facing_every_primary_is_negative(oracle):
    _, _, ref, (_n_s, n_t, _n_p), t = _frames(oracle, "behind_facing")
    assert n_t == W * HGT and np.all(t < 0)


def test_behind_away_is_seen_by_shadow_and_reflection_rays_only(oracle):
    """Measured: 37 pixels differ from the scene without the triangle."""
    img, _, ref, (_n_s, n_t, _n_p), _ = _frames(oracle, "behind_away")
    assert n_t == 0
    sc = F.behind_without()
    assert terms.exact_eq(sc, F.build("behind_away")[:-1]) and F.build("behind_away")[-1][0] == "triangle"
    bare = oracle.render(N.marshal(sc), W, HGT, F.depth("behind_away"), mode=oracle.MEMO)
    n = int((~np.all(_bits(img) == _bits(bare), axis=-1)).sum())
    print("behind_away: pixels that differ from the scene without the triangle:", n, flush=True)
    assert n >= 20


def test_zero_normal_triangle(oracle):
    """Measured (the triangle enlarged to v1 = (-1, -1, 4), v2 = 4 v1): 30 triangle primaries."""
    _, lv, ref, (_n_s, n_t, _n_p), _ = _frames(oracle, "zero_normal")
    assert n_t >= 25
    tri = ref["elem"] == 3
    assert int(tri.sum()) == n_t and not ref["normal"][tri].any()
    assert int((lv[tri] == 5).sum()) >= 25  # the chain re-hits the triangle down to the depth limit


@pytest.mark.parametrize("name", ["graze12", "graze16"])
def test_graze_hits_beyond_the_cull_extent(oracle, name):
    """Measured: largest primary t 28,966 (graze16: 463,412); 3064 pixels at level 5."""
    _, lv, _, _, t = _frames(oracle, name)
    assert t.max() > 1e4
    assert int((lv == 5).sum()) >= 2500


@pytest.mark.parametrize("name", ["pencil_wall", "pencil_fartri"])
def test_pencil_hits_half_a_million_units_away(oracle, name):
    """Measured: every primary t about 524,290; the wall's reflections reach levels 2 to 4 on 402
    pixels; the far triangle is lit (max channel 1.68)."""
    img, lv, _, (n_s, n_t, n_p), t = _frames(oracle, name)
    assert t.size == W * HGT and np.all(t > 5e5) and n_s == 0
    if name == "pencil_wall":
        assert n_p == W * HGT and int((lv >= 2).sum()) >= 300
    else:
        assert n_t == W * HGT and img.max() > 0.5


def test_empty_is_black(oracle):
    img, lv, _, kinds, _ = _frames(oracle, "empty")
    assert kinds == (0, 0, 0) and not img.any() and not lv.any()


@pytest.mark.parametrize("name", ["mesh_small", "big_flat"])
def test_small_mesh_and_big_flat_are_not_vacuous(oracle, name):
    """Measured: mesh_small 72 triangle primaries, 79 chains at level 5; big_flat 32 triangle and
    1680 plane primaries, 3059 chains at level 4."""
    _, lv, _, (_n_s, n_t, n_p), _ = _frames(oracle, name)
    assert n_t + n_p >= 50 and n_t >= 25
    assert int(lv.max()) >= 2


@pytest.mark.parametrize("name", ["tie3_tps", "zero_normal", "behind_facing", "corridor_nonunit", "mesh_small"])
def test_c_oracle_equals_term_restatement_on_flat_hostile_scenes(oracle, name):
    """Ties across kinds, the zero normal, negative distances and non-unit normals: the C oracle
    gives the term-level restatement's bits at 24x18, so these behaviours are the reference's own."""
    scene = F.build(name)
    el = N.marshal(scene)
    for d in (1, 3):
        a = oracle.render(el, 24, 18, d, mode=oracle.MEMO)
        b = _py(scene, 24, 18, d)
        assert np.array_equal(_bits(a), _bits(b)), f"{name} depth {d}"

"""The per-lane BVH walk of rt_query_rays and rt_query_shadow (k_query<.., SCAN_BVH>, rt_query.hip) on the
GPU, against the oracle in every byte: the batches of tests/bvh_batches.py, whose waves lie wholly in
the walk's domain — |o| <= 4 E per axis and |d.d - 1| <= 2^-20 — up to its limits and, one ray at a
time, just across them (such a wave takes the beam).  tests/test_query_bvh.py checks on the CPU what
each batch holds, and that a restatement of the walk gives the oracle's answers on them.

  C1  both memory layouts — s256 and s427 stage nodes and sphere rows in LDS, s428 and s2000 read them
      from HBM — and depths 10 to 13
  C2  trees with ties, twins, concentric and enclosing spheres, degenerate radii, flat objects scanned
      after the walk, 190 lights, and axis-parallel rays through bvh_inv's clamp in whole waves
  C3  wave composition: a ray's bytes do not depend on whether its wave walks
  C4  the loop iteration after stage_bvh, on walking waves
  C5  shadow queries through the walk
  C6  rt_update_scene across layouts and depths
  C7  trees of a few nodes (RT_BVH_MIN=2, read once per process: a child)

query, check, same, shadow and lit_equal are tests/test_gpu_query.py's, with their sentinel and guard
checks."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from eraytracer_amd import _native as N
from tests import bvh_batches as BB
from tests import bvh_ref as B
from tests import query_ref as Q
from tests.test_gpu_primary_tiles import Ctx
from tests.test_gpu_query import (ELEM_SENTINEL, PLANES, SENTINEL, check, lit_equal, query, query_device, same, shadow,
                                  to_device)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("f64", "f32")


def batches_of(name):
    """{batch name: (origins, directions, reference)} of a scene."""
    out = {"inside4E": BB.inside4E(name)[:3]}
    if name in BB.LAYOUT_SCENES:
        out["edge"] = BB.edge(name)[:3]
    if name == "lattice":
        out["axis"] = BB.axis()[:3]
    return out


@functools.lru_cache(maxsize=None)
def gpu_batches(name, cull=True):
    """{(batch name, precision): planes} of the scene's batches on one fresh context (computed once,
    read-only)."""
    out = {}
    with Ctx(Q.scene_of(name), cull=cull) as c:
        for what, (o, d, _) in batches_of(name).items():
            for prec in PRECS:
                out[what, prec] = Q._freeze(query(c, o, d, prec=prec))
    return out


def head(ref, n):
    return {k: ref[k][:n] for k in PLANES}


# ---- C1, C2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", BB.LAYOUT_SCENES + BB.HOSTILE_SCENES)
def test_walking_waves_equal_the_oracle(name, prec):
    """Batches 1 and 2 on the layout scenes, batch 1 on the hostile trees, batches 1 and 3 on the lattice:
    the oracle's bytes, and those of a context that tests every object."""
    for what, (o, d, ref) in batches_of(name).items():
        got = gpu_batches(name)[what, prec]
        print(name, what, prec, "hits", int((ref["elem"] >= 0).sum()), "walking waves",
              len(B.walking_waves(o, d, len(d), B.domain_E(name))), "of", (len(d) + 63) // 64, flush=True)
        check(got, ref, prec, what=f"{name} {what}")
        same(got, gpu_batches(name, cull=False)[what, prec], what=f"{name} {what} against brute force")


# ---- C3 -------------------------------------------------------------------------------------------
def with_far_rays(name, o, d):
    """The batch with a ray from 1e6 away put at a seeded lane of every wave of 64: (origins, directions,
    the positions of the batch's own rays, the positions of the far rays)."""
    rng = np.random.RandomState(BB.seed_of(name, 5))
    lo, hi = BB.box_of(name)
    n = len(d)
    waves = -(-n // 63)
    far = np.array([w * 64 + rng.randint(0, min(64, n + waves - w * 64)) for w in range(waves)])
    m = n + waves
    own = np.setdiff1d(np.arange(m), far)
    u = Q.unit_vectors(rng, waves)
    o2, d2 = np.empty((m, 3)), np.empty((m, 3))
    o2[own], d2[own] = o, d
    o2[far], d2[far] = (lo + hi) / 2 - 1e6 * u, u
    return o2, d2, own, far


@pytest.mark.parametrize("name", ["s256", "s428"])
def test_wave_composition(name):
    """Batch 1 as it is (every wave walks), with a far ray in every wave (every wave takes the beam),
    permuted, and as prefixes of 1, 63, 64, 65 and 257 rays — as n of the full arrays and as short
    arrays: the same bytes for the same ray, the oracle's.  And with every direction scaled to a length
    in [2^-3, 2^3] (no wave may walk: a walk would prune by distances that are not ray parameters)."""
    o, d, ref, _ = BB.inside4E(name)
    E = B.domain_E(name)
    whole = gpu_batches(name)["inside4E", "f64"]
    check(whole, ref, "f64", what=f"{name} inside4E")
    o2, d2, own, far = with_far_rays(name, o, d)
    assert len(B.walking_waves(o2, d2, len(d2), E)) == 0 and len(B.walking_waves(o, d, len(d), E)) == 41
    fref = Q.nearest_ref(Q.elems_of(name), o2[far], d2[far])
    rng = np.random.RandomState(BB.seed_of(name, 6))
    perm = rng.permutation(len(d))
    # the same rays with lengths in [2^-3, 2^3]: t is no longer the ray parameter the walk prunes by
    ds = np.ascontiguousarray(d * np.exp2(rng.uniform(-3, 3, size=(len(d), 1))))
    assert len(B.walking_waves(o, ds, len(ds), E)) == 0
    sref = Q.nearest_ref(Q.elems_of(name), o, ds)
    assert (sref["elem"] == ref["elem"]).mean() > 0.99
    with Ctx(Q.scene_of(name)) as c:
        got = query(c, o2, d2)
        same({k: got[k][own] for k in PLANES}, whole, what="a far ray in every wave")
        check({k: got[k][far] for k in PLANES}, fref, "f64", what="the far rays")
        check(query(c, o, ds), sref, "f64", what=f"{name} directions of other lengths")
        same(query(c, o[perm], d[perm]), {k: whole[k][perm] for k in PLANES}, what="permutation")
        for m in (1, 63, 64, 65, 257):
            same(query(c, o, d, n=m), head(whole, m), what=f"prefix {m}")
            same(query(c, o[:m], d[:m]), head(whole, m), what=f"batch of {m}")


@pytest.mark.parametrize("name", ["s256", "s428"])
def test_one_origin_on_the_walk(name):
    """RT_QUERY_ONE_ORIGIN from inside the box and from 3 E out on one axis: the repeated-origin call's
    bytes and the oracle's."""
    rng = np.random.RandomState(BB.seed_of(name, 8))
    E = B.domain_E(name)
    lo, hi = BB.box_of(name)
    inside = lo + (hi - lo) * rng.uniform(size=3)
    out = np.array([0.0, 3.0 * E, (lo[2] + hi[2]) / 2])
    with Ctx(Q.scene_of(name)) as c:
        for org in (inside, out):
            rep = np.tile(org, (BB.N_RAYS, 1))
            d = Q.unit_vectors(rng, BB.N_RAYS)
            aim = rng.uniform(size=BB.N_RAYS) < 0.6
            d[aim] = BB.aimed(rng, name, rep)[aim]
            d = np.ascontiguousarray(d)
            assert len(B.walking_waves(org, d, len(d), E)) == 41
            ref = Q.nearest_ref(Q.elems_of(name), org, d)
            share = (ref["elem"] >= 0).mean()
            print(name, org, "hit share %.2f" % share, flush=True)
            assert 0.1 <= share <= 0.95
            for prec in PRECS:
                one = query(c, org, d, prec=prec)
                check(one, ref, prec, what=f"{name} one origin {org}")
                same(one, query(c, rep, d, prec=prec), what="one origin against a repeated one")


# ---- C4 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s256", "s428"])
def test_loop_after_staging(name):
    """2^21 + 64 * 5 + 37 rays — 8192 blocks of 256 and six more waves, the last one partial — tiling
    batch 1: the tiling of its planes (GPU against GPU), and nothing past n."""
    import torch
    o, d, ref, _ = BB.inside4E(name)
    small = gpu_batches(name)["inside4E", "f64"]
    check(small, ref, "f64", what=f"{name} inside4E")
    n = (1 << 21) + 64 * 5 + 37
    assert 8192 * 256 < n < 8192 * 256 + 256 * 2
    idx = torch.arange(n, device="cuda") % len(d)
    d_o, d_d = to_device(o)[idx].contiguous(), to_device(d)[idx].contiguous()
    with Ctx(Q.scene_of(name)) as c:
        buf, _ = query_device(c, d_o, d_d, n, one=False)
    for k in PLANES:
        want = to_device(small[k])[idx]
        ibits = torch.int32 if k == "elem" else torch.int64
        assert torch.equal(buf[k][:n].contiguous().view(ibits), want.contiguous().view(ibits)), k
        assert bool((buf[k][n:] == (ELEM_SENTINEL if k == "elem" else SENTINEL)).all()), (k, "entries past n written")


# ---- C5 -------------------------------------------------------------------------------------------
def test_shadow_queries_on_the_walk():
    """Shadow rays are unit vectors from the lights: the three shadow batches in one call each, three
    lights of s300l190+g with RT_QUERY_ONE_ORIGIN, and s2000 with every object tested."""
    L, H, E, ref = BB.shadows_s2000()
    print("s2000", len(ref), "lit", int(ref.sum()), flush=True)
    with Ctx(Q.scene_of("s2000")) as c:
        lit_equal(shadow(c, L, H, E), ref, "s2000")
    with Ctx(Q.scene_of("s2000"), cull=False) as c:
        lit_equal(shadow(c, L, H, E), ref, "s2000 brute force")
    L, H, E, ref, parts = BB.shadows_l190()
    print("s300l190+g", len(ref), "lit", int(ref.sum()), flush=True)
    with Ctx(Q.scene_of("s300l190+g")) as c:
        lit_equal(shadow(c, L, H, E), ref, "s300l190+g")
        for i in (0, 77, 189):
            p = parts[i]
            lit_equal(shadow(c, L[p.start], H[p], E[p]), ref[p], f"s300l190+g light {i}, one origin")
    L, H, E, ref, _ = BB.shadows_twins160()
    print("s160+g", len(ref), "lit", int(ref.sum()), flush=True)
    with Ctx(Q.scene_of("s160+g")) as c:
        lit_equal(shadow(c, L, H, E), ref, "s160+g twins")


# ---- C6 -------------------------------------------------------------------------------------------
def test_scene_updates_across_layouts():
    """One context through s256 (staged, depth 10), s2000 (HBM, 13), s64 (no BVH), s428 (HBM, 11), s427
    (staged, 11) and the lattice by rt_update_scene: after each step a 640-ray prefix of the scene's
    batch equals the oracle; then a shadow batch."""
    m = 640
    with Ctx(Q.scene_of("s256")) as c:
        for step, name in enumerate(("s256", "s2000", "s64", "s428", "s427", "lattice")):
            if step:
                el = Q.elems_of(name)
                N.check(c.L.rt_update_scene(c.p, el, len(el)), "rt_update_scene")
            o, d, ref = Q.incoherent(name)[:3] if name == "s64" else BB.inside4E(name)[:3]
            check(query(c, o[:m], d[:m]), head(ref, m), "f64", what=f"step {step}: {name}")
        L, H, E, ref, _ = Q.shadows("lattice", 64, 48, 2)
        assert len(ref) >= 1000 and 0.1 <= ref.mean() <= 0.9
        lit_equal(shadow(c, L[:2000], H[:2000], E[:2000]), ref[:2000], "shadow queries after five updates")


# ---- C7 -------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
from tests import query_ref as Q
from tests.test_gpu_primary_tiles import Ctx
from tests.test_gpu_query import PLANES, check, lit_equal, query, shadow
refs = np.load(sys.argv[1])
ran = 0
for name in sys.argv[2].split(","):
    with Ctx(Q.scene_of(name)) as c:
        for what in ("unit", "domain", "ties"):
            if f"{name}|{what}|o" not in refs:
                continue
            o, d = refs[f"{name}|{what}|o"], refs[f"{name}|{what}|d"]
            ref = {k: refs[f"{name}|{what}|{k}"] for k in PLANES}
            for prec in ("f64", "f32"):
                check(query(c, o, d, prec=prec), ref, prec, what=f"{name} {what}")
                ran += 1
        if name == "twins":
            light, H, E, lit = (refs[f"twins|shadow|{k}"] for k in ("light", "H", "E", "lit"))
            lit_equal(shadow(c, light, H, E), lit, "twins shadows")
            ran += 1
print("tiny ok", ran)
"""


def test_tiny_trees(tmp_path):
    """RT_BVH_MIN=2: twins (4 spheres), s2+ties (7), mixed (48, with triangles and planes), default (3, with
    a triangle and a plane) and s7+g (19) get a BVH, and their unit rays walk it: batch-1-style rays,
    Q.domain's batch with its hostile slots, rays that hit G's mirrored pair at exactly equal distances
    (in s7+g the walk visits the later sphere first), and the twins' shadow batch with its entries lit
    only because two elements are the same term."""
    arrs = {}
    for name in BB.TINY_SCENES:
        o, d = BB.unit_rays(name)
        sets = {"unit": (o, d, Q.nearest_ref(Q.elems_of(name), o, d))}
        if name in Q.SEEDS:
            sets["domain"] = Q.domain(name)[:3]
        if name in BB.TIE_SCENES:
            sets["ties"] = BB.tie_rays(name)
        for what, (o, d, ref) in sets.items():
            arrs[f"{name}|{what}|o"], arrs[f"{name}|{what}|d"] = o, d
            for k in PLANES:
                arrs[f"{name}|{what}|{k}"] = ref[k]
    light, H, E, lit, by_index = Q.duplicate_shadows()
    assert ((lit == 1) & (by_index == 0)).any()
    arrs.update({"twins|shadow|light": light, "twins|shadow|H": H, "twins|shadow|E": E, "twins|shadow|lit": lit})
    path = str(tmp_path / "refs.npz")
    np.savez(path, **arrs)
    env = dict(os.environ, PYTHONPATH=ROOT, RT_BVH_MIN="2")
    r = subprocess.run([sys.executable, "-c", _CHILD, path, ",".join(BB.TINY_SCENES)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tiny ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split("tiny ok")[1].split()[0]) == 2 * (5 + 3 + 2) + 1

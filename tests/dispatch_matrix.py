"""Where every kernel instantiation of csrc/rt_render.hip is tested.

rt_render.hip compiles 183 kernel instantiations, and rt_launch_rows, wave_level_lists, wave_reflect
and wave_walks pick among them at run time.  This module says, for each one, exactly one of:

* ``("case", name)``: matrix case ``name`` (CASES below) launches it, and tests/test_gpu_dispatch_matrix.py
  renders that case, reads the context's launch record (rt_debug_launched) and fails unless the record
  holds the instantiation; every frame of the case is compared with brute force, the other precision
  and the oracle;
* ``("elsewhere", test)``: not a render kernel; the named test runs it against its own reference.

No instantiation is compiled that the dispatch code cannot select.

tests/test_dispatch_matrix.py builds the list of instantiations itself (the host stubs of a host-only
compile) and fails on a stub this module does not classify, on an entry without a stub and on an entry
classified twice: a kernel added later fails it until someone says here where it is tested.

Names are spelled as ``nm -C`` spells the host stubs and as rt_debug_launched spells the record:
``k_walk<1, true, 2, 1, true>``.  PREC is 0 (binary64 frames) or 1 (binary32), SPH 0 (any
scene), 1 (spheres only) or 2 (spheres only, tables staged in LDS); k_walk's SRC says where an
ancestor's shadow answers come from: 0 tested again, 1 k_light's array, 2 the child's record.

The scenes.  Every case is rendered with integer specular powers (hostile.unit_powers: 0 and 1, where
pow is exact in glibc and in the kernels, so the frame equals the oracle's bit for bit) and with general
powers (GENPOW kernels: the device's pow is compiled in).  The general-power spheres-only scenes are
scenes.named(...) with every sphere's power replaced in list order by P[rng % 7], rng =
SplitMix64(0xA5A5): non-integers and 1025 beside 0, 1, 4 and 20 on purpose, so that waves mix lanes
that leave pow_libm through pow() with lanes that take the binary powering.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from eraytracer_amd import scenes
from eraytracer_amd.records import material
from tests import hostile

P = (1, 4, 20, 0.5, 2.5, 0, 1025)
# the same scenes with every power an integer in 0..1024 (what P is compared with to show that pow mattered)
P_INTEGER = (1, 4, 20, 1, 3, 0, 1024)
POWER_SEED = 0xA5A5


def general_powers(scene, powers=P):
    """`scene` with every sphere's specular power replaced, in list order, by powers[rng.next_u64() % 7]."""
    rng = scenes.SplitMix64(POWER_SEED)
    out = []
    for t in scene:
        if t[0] == "sphere":
            m = t[3]
            t = t[:3] + (material(m[1], powers[rng.next_u64() % len(powers)], m[3], m[4]),)
        out.append(t)
    return out


def relit(scene, m):
    """`scene` with its point lights replaced by the m lights of a synthetic scene."""
    lights = [t for t in scenes.synthetic_scene(48, 0x5EED0048, n_lights=m) if t[0] == "point_light"]
    k = next(i for i, t in enumerate(scene) if t[0] == "point_light")
    rest = [t for t in scene if t[0] != "point_light"]
    return rest[:k] + lights + rest[k:]


# name -> (builder of the base scene, spheres only).  What makes each one take its kernels:
#   s64, s64l8  staged (SPH 2), per-light terms of 64 and 128 bytes (walk_fold)
#   s64l9       staged, more lights than TERM_MAX_LIGHTS: no terms
#   s20l33      staged with more than 32 lights (shadow answers do not fit the records: SRC 0)
#   s64l10      the first light count at which S64's tables no longer fit LDS_STAGE_MAX: SPH 1, no BVH
#   s64l40      SPH 1, more than 32 lights
#   s256        SPH 1, the BVH from reflection level 2 (its natural level)
#   mixed       spheres, triangles and planes: SPH 0 (its own powers are general already; mixed_int's
#               too: synthetic_mixed's last triangle and plane have the powers 2.5 and 0.5 whatever
#               `powers` says, so mixed_int has never been an integer-power scene)
#   mixedl40    mixed with 40 lights
#   default     the reference's scene: 5 objects, no wave beams (NB)
BASES = {
    "s64": (lambda: scenes.named("s64"), True),
    "s64l8": (lambda: scenes.named("s64l8"), True),
    "s64l9": (lambda: scenes.named("s64l9"), True),
    "s20l33": (lambda: scenes.named("s20l33"), True),
    "s64l10": (lambda: scenes.named("s64l10"), True),
    "s64l40": (lambda: scenes.named("s64l40"), True),
    "s256": (lambda: scenes.named("s256"), True),
    "mixed": (lambda: scenes.named("mixed"), False),
    "mixed_int": (lambda: scenes.named("mixed_int"), False),
    "mixedl40": (lambda: relit(scenes.named("mixed"), 40), False),
    "default": (lambda: scenes.named("default_powers"), False),
}


def scene(base, powers):
    """powers: 'gen' (general: GENPOW kernels), 'int' (0 and 1: exact on both sides) or 'alt' (the
    general scene with P_INTEGER's powers in place of P's: the vacuity test's comparison)."""
    build, sph = BASES[base]
    sc = build()
    if powers == "int":
        return hostile.unit_powers(sc)
    if sph:
        return general_powers(sc, P if powers == "gen" else P_INTEGER)
    if powers == "gen":
        return sc
    # the mixed and default scenes' own general powers, made integers: 0.5 -> 1, 2.5 -> 3, 1025 -> 1024
    swap = {0.5: 1, 2.5: 3, 1025: 1024}
    return [t[:-1] + (material(t[-1][1], swap.get(t[-1][2], t[-1][2]), t[-1][3], t[-1][4]),)
            if t[0] in ("sphere", "triangle", "plane") else t for t in sc]


def n_lights(sc):
    return sum(1 for t in sc if t[0] == "point_light")


# ---- the colour bound against the oracle ----------------------------------------------------------
def colour_bound(lights, depth):
    """The relative bound on |gpu - oracle| per channel of a general-power frame: 2^-52 (2 + 2 (L + 5) D).

    The geometry is bit-identical, so both sides call pow on the same operands; glibc's result is
    within 0.52 ulp and the device's within 1 ulp of the true value.  Every term of shade() is
    non-negative (colours in [0, 1], both dot products through max0, shininess, reflectivity and the
    shadow factor >= 0; checked in rt_shade.inc and oracle/rt_oracle.c), so a colour is a sum of
    non-negative terms without cancellation, and between sp and a level's result lie about L + 5
    separately rounded operations, each of which can move a perturbed value by one more ulp, at each
    of D levels.  The factor 2 is the margin over that worst case."""
    return 2.0 ** -52 * (2 + 2 * (lights + 5) * depth)


def colour_excess(gpu, ref, lights, depth):
    """(worst, bad): the largest |gpu - ref| / max(|gpu|, |ref|) in units of 2^-52 over the channels
    where ref is not +-0, and the number of channels outside the bound (where ref is +-0: any
    difference at all)."""
    gpu, ref = np.asarray(gpu, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    diff = np.abs(gpu - ref)
    scale = np.maximum(np.abs(gpu), np.abs(ref))
    zero = ref == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(scale > 0, diff / scale, 0.0)
    bad = np.where(zero, diff != 0, ~(diff <= colour_bound(lights, depth) * scale))
    worst = float(rel[~zero].max()) * 2.0 ** 52 if (~zero).any() else 0.0
    return worst, int(bad.sum())


# ---- the cases ------------------------------------------------------------------------------------
# A frame of a case: the base scene, the size and depth, side streams on or off, levels requested or
# not, samples per pixel, RT_ORDER_EXACT (0) or RT_ORDER_FAST (1).
Frame = namedtuple("Frame", "base w h depth side levels spp order", defaults=(1, False, 1, 0))
SPP_SEED = 0x5EED0007

# A case: the child it renders in (one per environment: the RT_* variables are read once per process),
# its frames, and the instantiations it owns.  Every case is rendered four times: PREC 0 and 1, integer
# and general powers; a claim is a template over {P} and {G} and belongs to the instance with those
# values — "k_light<{P}, {G}, 2>" is four instantiations, one per instance; a claim without {P} belongs
# to the PREC 0 instances alone and one without {G} to the integer-power instances alone (k_items: to
# the one that is both).  An instance that owns nothing is not rendered.
Case = namedtuple("Case", "name child frames claims")

ENV = {
    "wave": {"RT_ENGINE": "wave"},
    "bvh": {"RT_ENGINE": "wave", "RT_BVH_MIN": "2", "RT_BVH_LEVEL": "1"},
    "fused": {"RT_ENGINE": "fused"},
}

S64, S64L8 = ("s64", 96, 96), ("s64l8", 96, 96)
S64L9, S64L10, S64L40, S20L33 = ("s64l9", 64, 48), ("s64l10", 64, 48), ("s64l40", 64, 48), ("s20l33", 128, 96)
S256, MIXED, MIXEDL40, DEFAULT = ("s256", 64, 48), ("mixed", 128, 96), ("mixedl40", 64, 48), ("default", 64, 48)


def _side(sph, many, few, few_spp):
    """Side streams on: k_light shades levels 0 and 1 beside the reflection chain (k_reflect), k_walk
    finishes the chains ending at level 1 and then the rest, k_walk_deep the deep levels (depth >= 3);
    with more than 32 lights the walks test the shadows again (SRC 0); a supersampled frame sums its
    samples with k_accum."""
    return Case(f"sph{sph}-side", "wave",
                [Frame(*few, 5 if few[0] != "s256" else 8), Frame(*many, 3 if sph == 2 else 4),
                 Frame(*few_spp, 4, spp=3)],
                [f"k_light<{{P}}, {{G}}, {sph}>", f"k_walk<{{P}}, {{G}}, {sph}, 1, false>",
                 f"k_walk<{{P}}, {{G}}, {sph}, 0, false>", f"k_walk_deep<{{G}}, {sph}>"])


def _levels(sph, many, few):
    """Side streams off with levels requested: k_reflect<LEVELS>, k_light, and one merged k_walk."""
    return Case(f"sph{sph}-levels", "wave",
                [Frame(*few, 5 if few[0] != "s256" else 8, side=0, levels=True),
                 Frame(*many, 3 if sph == 2 else 4, side=0, levels=True)],
                [f"k_walk<{{P}}, {{G}}, {sph}, 1, true>", f"k_walk<{{P}}, {{G}}, {sph}, 0, true>"])


def _depth2(sph, *scenes_):
    """Side streams off, no levels, depth 2: k_reflect_shade<!ILP> and the walk that finds the shadow
    answers in the children's records (SRC 2)."""
    return Case(f"sph{sph}-depth2", "wave", [Frame(*s, 2, side=0) for s in scenes_],
                [f"k_reflect_shade<{{P}}, {{G}}, {sph}, false, false, false>",
                 f"k_walk<{{P}}, {{G}}, {sph}, 2, true>"])


CASES = [
    # ---- SPH 2: spheres only, tables staged in LDS --------------------------------------------------
    _side(2, S20L33, S64, S64L8),
    _levels(2, S20L33, S64),
    _depth2(2, S64, S64L8),
    # depth 3 (the LAST launch is launch 2) and deeper, with the terms of 64 and 128 bytes folded, with
    # more lights than terms are kept for, and with more than 32 (no inline walks: no LAST)
    Case("sph2-inline", "wave",
         [Frame(*S64, 3, side=0), Frame(*S64, 5, side=0), Frame(*S64L8, 5, side=0), Frame(*S64L9, 4, side=0),
          Frame(*S20L33, 3, side=0), Frame(*S64L8, 4, side=0, spp=3)],
         ["k_reflect_shade<{P}, {G}, 2, true, false, false>", "k_reflect_shade<{P}, {G}, 2, true, false, true>"]),
    # what does not depend on the scene class is claimed once, by the S64 frames with side streams
    Case("wave-common", "wave",
         [Frame(*S64, 5), Frame(*S64, 5, levels=True), Frame(*S64, 4, spp=3)],
         ["k_primary<{P}, false>", "k_primary<{P}, true>", "k_accum<{P}>", "k_reflect<false, false>",
          "k_reflect<false, true>", "k_reflect<true, false>", "k_reflect<true, true>", "k_pmask<false>",
          "k_pmask<true>", "k_items"]),
    # ---- SPH 1: spheres only, tables in L2 ----------------------------------------------------------
    _side(1, S64L40, S256, S256),
    _levels(1, S64L40, S256),
    _depth2(1, S256, S64L10),
    # S256: level 1 on the wave beams, levels >= 2 through the BVH; s64l10: no BVH; s64l40: no LAST
    Case("sph1-inline", "wave",
         [Frame(*S256, 8, side=0), Frame(*S256, 3, side=0), Frame(*S64L10, 4, side=0), Frame(*S64L10, 3, side=0),
          Frame(*S64L40, 4, side=0), Frame(*S256, 4, side=0, spp=3)],
         ["k_reflect_shade<{P}, {G}, 1, true, false, false>", "k_reflect_shade<{P}, {G}, 1, true, false, true>",
          "k_reflect_shade<{P}, {G}, 1, true, true, false>"]),
    # the BVH from level 1 on, so also in the LAST launch of depth 3
    Case("sph1-bvh", "bvh", [Frame(*S64L10, 3, side=0), Frame(*S64L10, 4, side=0)],
         ["k_reflect_shade<{P}, {G}, 1, true, true, true>"]),
    # ---- SPH 0: any scene ---------------------------------------------------------------------------
    _side(0, MIXEDL40, MIXED, MIXED),
    _levels(0, MIXEDL40, MIXED),
    _depth2(0, MIXED),
    Case("sph0-inline", "wave",
         [Frame(*MIXED, 5, side=0), Frame(*MIXED, 3, side=0), Frame(*MIXEDL40, 4, side=0),
          Frame("mixed_int", 128, 96, 5, side=0)],
         ["k_reflect_shade<{P}, {G}, 0, true, false, false>", "k_reflect_shade<{P}, {G}, 0, true, false, true>"]),
    Case("sph0-bvh", "bvh", [Frame(*MIXED, 5, side=0), Frame(*MIXED, 3, side=0)],
         ["k_reflect_shade<{P}, {G}, 0, true, true, false>", "k_reflect_shade<{P}, {G}, 0, true, true, true>"]),
    # ---- the fused engine (forced): both orders, levels on and off, with wave beams and without ------
    Case("fused-beams", "fused",
         [Frame(*S64, 5, order=o, levels=lv) for o in (0, 1) for lv in (False, True)],
         [f"k_render<{o}, {{P}}, {lv}, {{G}}, false>" for o in (0, 1) for lv in ("false", "true")]),
    Case("fused-nobeams", "fused",
         [Frame(*DEFAULT, 5, order=o, levels=lv) for o in (0, 1) for lv in (False, True)],
         [f"k_render<{o}, {{P}}, {lv}, {{G}}, true>" for o in (0, 1) for lv in ("false", "true")]),
]

PRECS = (0, 1)
POWERS = ("int", "gen")


def instances(case):
    """The four renderings of a case: (instance name, PREC, powers)."""
    return [(f"{case.name}/{'f64' if p == 0 else 'f32'}/{g}", p, g) for p in PRECS for g in POWERS]


def claims(case, prec, powers):
    """The instantiations the (prec, powers) rendering of `case` must launch."""
    out = []
    for c in case.claims:
        if ("{P}" not in c and prec != 0) or ("{G}" not in c and powers != "int"):
            continue
        out.append(c.format(P=prec, G="true" if powers == "gen" else "false"))
    return out


# ---- the other class --------------------------------------------------------------------------------
ELSEWHERE = {
    **{f"k_eval_math<{op}>": "tests/test_gpu_math_exact.py (rt_eval_math, op %d)" % op for op in range(7)},
    "k_selftest_math": "tests/test_gpu_parity.py::test_selftest_math (rt_selftest_math)",
}


def table():
    """instantiation -> list of its classifications (the CPU test wants exactly one each)."""
    t = {}
    for case in CASES:
        for inst, p, g in instances(case):
            for c in claims(case, p, g):
                t.setdefault(c, []).append(("case", inst))
    for k, why in ELSEWHERE.items():
        t.setdefault(k, []).append(("elsewhere", why))
    return t


def general_frames():
    """Every (base, w, h, depth, spp) a general-power rendering uses: what the vacuity test checks."""
    return sorted({(f.base, f.w, f.h, f.depth, f.spp) for case in CASES for f in case.frames})


# ---- the child process of tests/test_gpu_dispatch_matrix.py ------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def child_main(job_path):
    """Render the instances listed in the JSON file `job_path` in this process (whose RT_* environment
    the parent chose) and check every frame; print one JSON line per instance: its launch record and
    its largest distance from the oracle.  The job: {"instances": [[case name, prec, powers], ...],
    "save": an .npz to write the binary64 frames of RT_ORDER_EXACT to, or null, "other": an .npz of
    the other engine's, or null}."""
    import ctypes
    import json

    import torch

    from eraytracer_amd import _native as N
    from oracle import oracle as O

    with open(job_path) as fh:
        job = json.load(fh)
    L = N.lib()
    cases = {c.name: c for c in CASES}
    other = dict(np.load(job["other"])) if job.get("other") else {}
    saved, brutes, refs = {}, {}, {}

    def launch(p, f, prec):
        rows = L.rt_shard_rows(f.h, 16, 1)
        img = torch.full((rows, f.w, 3), float("nan"), dtype=torch.float64 if prec == 0 else torch.float32, device="cuda")
        lv = torch.full((rows, f.w), 255, dtype=torch.uint8, device="cuda") if f.levels else None
        N.check(L.rt_launch_spp(p, f.w, f.h, f.depth, 16, 0, 1, prec, f.order, f.spp, SPP_SEED, img.data_ptr(),
                                lv.data_ptr() if f.levels else None, torch.cuda.current_stream().cuda_stream),
                "rt_launch_spp")
        torch.cuda.synchronize()
        return img.cpu().numpy()[:f.h], (lv.cpu().numpy()[:f.h] if f.levels else None)

    def context(sc, side, cull):
        el = N.marshal(sc)
        p = ctypes.c_void_p()
        N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
        N.check(L.rt_configure(p, N.RT_CFG_SIDE_STREAMS, side))
        if not cull:
            N.check(L.rt_configure(p, N.RT_CFG_CULL, 0))
        return p

    for name, prec, powers in job["instances"]:
        case, record, worst = cases[name], set(), 0.0
        for f in case.frames:
            what = f"{name} {'f64' if prec == 0 else 'f32'} {powers} {tuple(f)}"
            sc = scene(f.base, powers)
            nl = n_lights(sc)
            p = context(sc, f.side, True)
            try:
                N.launched(p, reset=True)  # (a fresh context's record is empty; reset all the same)
                got, lv = launch(p, f, prec)
                record |= N.launched(p)
            finally:
                L.rt_release(p)
            assert np.all(np.isfinite(got)), what
            # brute force: no filters, hence the SPH 0 kernels (or the fused kernel without beams), side streams on
            key = (f.base, powers, f.w, f.h, f.depth, f.spp, f.order, f.levels)
            if key not in brutes:
                p = context(sc, 1, False)
                try:
                    brutes[key] = launch(p, f, 0)
                finally:
                    L.rt_release(p)
            brute, blv = brutes[key]
            assert same_bits(got, brute if prec == 0 else brute.astype(np.float32)), \
                (what, "differs from brute force", int((got != brute.astype(got.dtype)).any(axis=-1).sum()))
            if f.levels:
                assert same_bits(lv, blv), (what, "levels differ from brute force")
            # the other engine (binary64, the reference's order)
            okey = "|".join(str(x) for x in (f.base, powers, f.w, f.h, f.depth))
            if prec == 0 and f.order == 0 and f.spp == 1:
                saved[okey] = got
                if okey in other:
                    assert same_bits(got, other[okey]), (what, "differs from the other engine")
            # the oracle, against the binary64 frame (the binary32 one is that frame rounded)
            rkey = key[:6]
            if rkey not in refs:
                refs[rkey] = O.render(N.marshal(sc), f.w, f.h, f.depth, mode=O.MEMO, levels=True, spp=f.spp, seed=SPP_SEED)
            ref, rlv = refs[rkey]
            if f.levels:
                assert same_bits(lv, rlv), (what, "levels differ from the oracle", int((lv != rlv).sum()))
            err = float(np.abs(brute - ref).max())
            assert err <= 1e-5, (what, "max |delta|", err)
            if powers == "int" and f.order == 0:
                n = int((brute.view(np.int64) != ref.view(np.int64)).any(axis=-1).sum())
                assert n == 0, (what, f"{n} pixels not bit-identical to the oracle")
            else:  # general powers; or RT_ORDER_FAST, the same non-negative terms summed in another order
                w, bad = colour_excess(brute, ref, nl, f.depth)
                print(f"{what}: largest |gpu - ref| / max(|gpu|, |ref|) = {w:.2f} x 2^-52, bound "
                      f"{colour_bound(nl, f.depth) * 2.0 ** 52:.0f}", flush=True)
                assert bad == 0, (what, f"{bad} channels outside the bound", w)
                if f.order == 0:
                    worst = max(worst, w)
        print("RECORD " + json.dumps({"case": name, "prec": prec, "powers": powers, "record": sorted(record),
                                      "worst": worst}), flush=True)
    if job.get("save"):
        np.savez(job["save"], **saved)
    print("matrix ok", flush=True)

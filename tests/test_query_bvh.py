"""The ray queries' BVH walk on the CPU: tests/bvh_ref.py restates bvh_domain, bvh_inv, bvh_slab2 and
scan_bvh in the kernel's number formats over the node table the library's scene compiler built
(tests/csrc/bvh_dump.cpp, under AddressSanitizer and UBSan), and every in-domain ray of the batches of
tests/bvh_batches.py must get the oracle's element and distance bits from it — at the kernel's slab
tolerance and at half of it, with the reciprocal moved an ulp either way.  A disagreement on an
in-domain ray is a hole in the proof at the top of rt_query.hip, not a test to be loosened.

The rest checks, on the reference alone, that each batch tests/test_gpu_query_bvh.py sends holds what
it is built for."""
import numpy as np
import pytest

from eraytracer_amd import _native as N
from tests import bvh_batches as BB
from tests import bvh_ref as B
from tests import query_ref as Q

# scene: (n_sph, bvh_depth) with the default environment
COMPILED = {"s256": (256, 10), "s427": (427, 11), "s428": (428, 11), "s2000": (2000, 13), "s160+g": (172, 10),
            "s160+d": (177, 10), "s300l190+g": (312, 11), "lattice": (175, 10), "big_flat": (160, 10)}
WALKS = [(2.0 ** -16, 0), (2.0 ** -16, -1), (2.0 ** -16, 1), (2.0 ** -17, 0), (2.0 ** -17, -1), (2.0 ** -17, 1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def kinds_of(name):
    return np.array([e.kind for e in Q.elems_of(name)])


# ---- the compiled trees ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COMPILED))
def test_compiled_tree(name):
    b = B.dump(name)
    assert b["bvh_ok"] == 1 and b["cull_ok"] == 1
    assert (b["n_sph"], b["depth"]) == COMPILED[name]
    assert b["n_bvh"] == b["n_sph"] - 1 and b["depth"] <= 18
    assert b["ext"] == B.scene_ext(Q.elems_of(name)), "tests/bvh_ref.py's scene_ext is not SceneHdr::ext"
    # every sphere is a leaf once, every node but the root a child once, the ids are the leaves' compact ids
    links = b["links"].ravel()
    leaves, inner = ~links[links < 0], links[links >= 0]
    assert sorted(leaves.tolist()) == list(range(b["n_sph"]))
    assert sorted(inner.tolist()) == list(range(1, b["n_bvh"]))
    assert (b["ids"].ravel()[links >= 0] == -1).all()
    ids = b["ids"].ravel()[links < 0]
    assert ((ids >= 0) & (ids < b["n_obj"])).all() and len(set(ids.tolist())) == b["n_sph"]
    assert (kinds_of(name)[b["elem_of"][ids]] == N.RT_SPHERE).all()
    assert (b["nodes"][:, 0:6] < b["nodes"][:, 6:12]).all()


def test_the_two_layouts_straddle_the_staging_limit():
    """rt_query_launch stages nodes and sphere rows in LDS when 64 (n - 1) + 32 n <= BVH_LDS_MAX."""
    for name, staged in (("s256", True), ("s427", True), ("s428", False), ("s2000", False)):
        b = B.dump(name)
        size = b["n_bvh"] * B.NODE_BYTES + b["n_sph"] * B.ROW_BYTES
        assert size == 96 * b["n_sph"] - 64
        assert (size <= B.BVH_LDS_MAX) == staged, (name, size)
    assert 96 * 427 - 64 == 40928 and B.BVH_LDS_MAX == 40960


def test_tiny_trees_exist_only_when_forced():
    for name in BB.TINY_SCENES:
        assert B.dump(name)["bvh_ok"] == 0, name
        b = B.dump(name, 2)
        assert b["bvh_ok"] == 1 and b["n_bvh"] == b["n_sph"] - 1 >= 1, name


# ---- the restatement against the oracle ----------------------------------------------------------
def batches_of(name):
    out = [("inside4E", BB.inside4E(name)[:3]), ("edge", BB.edge(name)[:3])]
    if name == "lattice":
        out.append(("axis", BB.axis()[:3]))
    return out


@pytest.mark.parametrize("name", BB.SPHERE_SCENES)
def test_walk_equals_the_oracle(name):
    """Every in-domain ray of batches 1 to 3: the oracle's elem and t bits, for rcp_ulp in {-1, 0, 1} at
    the kernel's tolerance and at half of it (the proof needs (1 + 2^-20)(1 + 2^-21) < 1 + 2^-19)."""
    b, E = B.dump(name), B.domain_E(name)
    for what, (o, d, ref) in batches_of(name):
        ind = B.in_domain(o, d, E)
        oi, di = o[ind], d[ind]
        for tol, ulp in WALKS:
            elem, t, top, visits, pruned = B.walk(b, oi, di, tol=tol, rcp_ulp=ulp)
            bad = np.flatnonzero((elem != ref["elem"][ind]) | (bits(t) != bits(ref["t"][ind])))
            print(name, what, "tol 2^%d" % np.log2(tol), "rcp_ulp", ulp, "rays", int(ind.sum()), "most stack entries",
                  int(top.max()), "most visits", int(visits.max()), "pruned pops", int(pruned.sum()), flush=True)
            assert not len(bad), (f"{name} {what} tol {tol} rcp_ulp {ulp}: {len(bad)} in-domain rays differ from the "
                                  f"oracle, first ray {np.flatnonzero(ind)[bad[0]]}: walk ({elem[bad[0]]}, {t[bad[0]]!r}) "
                                  f"against ({ref['elem'][ind][bad[0]]}, {ref['t'][ind][bad[0]]!r})")
            assert pruned.sum() > 0, "no popped entry was pruned by tlim"
            if name == "s2000":
                assert top.max() >= 8, "no ray holds 8 stack entries"
            assert top.max() <= b["depth"] - 1


def test_walk_on_a_scene_with_flat_objects():
    """big_flat: the walk sees the spheres only (the kernel scans triangles and planes after it): the
    oracle's hit where that is a sphere, and nothing nearer where it is not."""
    name = "big_flat"
    b, E = B.dump(name), B.domain_E(name)
    kind = kinds_of(name)
    for what, (o, d, ref) in batches_of(name):
        ind = B.in_domain(o, d, E)
        sph = (ref["elem"] >= 0) & (kind[np.where(ref["elem"] >= 0, ref["elem"], 0)] == N.RT_SPHERE)
        for tol, ulp in WALKS:
            elem, t, top, _, pruned = B.walk(b, o[ind], d[ind], tol=tol, rcp_ulp=ulp)
            s = sph[ind]
            assert (elem[s] == ref["elem"][ind][s]).all() and (bits(t[s]) == bits(ref["t"][ind][s])).all(), (what, tol, ulp)
            assert (t[~s] >= ref["t"][ind][~s]).all(), (what, tol, ulp)  # (a miss: inf against inf)
            assert pruned.sum() > 0
        print(name, what, "sphere hits", int(sph.sum()), "most stack entries", int(top.max()), flush=True)


@pytest.mark.parametrize("name", BB.TINY_SCENES)
def test_walk_on_tiny_trees(name):
    """RT_BVH_MIN=2: trees of 2 to 47 nodes; the sphere part of the oracle's answer as on big_flat."""
    b, E = B.dump(name, 2), B.domain_E(name)
    kind = kinds_of(name)
    o, d = BB.unit_rays(name)
    assert B.in_domain(o, d, E).all()
    ref = Q.nearest_ref(Q.elems_of(name), o, d)
    sph = (ref["elem"] >= 0) & (kind[np.where(ref["elem"] >= 0, ref["elem"], 0)] == N.RT_SPHERE)
    assert sph.sum() >= 100
    for tol, ulp in WALKS:
        elem, t, _, _, _ = B.walk(b, o, d, tol=tol, rcp_ulp=ulp)
        assert (elem[sph] == ref["elem"][sph]).all() and (bits(t[sph]) == bits(ref["t"][sph])).all(), (tol, ulp)
        if b["n_tri"] + b["n_pl"] == 0:
            assert (elem == ref["elem"]).all() and (bits(t) == bits(ref["t"])).all(), (tol, ulp)


def test_tie_rays_tell_a_walk_without_the_list_order_rule():
    """Exact distance ties between G's mirrored pair, in trees of 6 and 18 nodes (RT_BVH_MIN=2): the walk
    gives the oracle's element, the earlier of the two; a walk whose leaf test takes `t < bt` alone — the
    first of the two it happens to visit — gets s7+g wrong (in s2+ties, as in s160+g, it visits the
    earlier one first)."""
    wrong = {}
    for name in BB.TIE_SCENES:
        b, E = B.dump(name, 2), B.domain_E(name)
        o, d, ref = BB.tie_rays(name)
        assert B.in_domain(o, d, E).all() and len(B.walking_waves(o, d, len(d), E)) == BB.N_TIES // 64
        assert (o[:, 0] == 0).all() and (d[:, 0] == 0).all() and ref["ties"].sum() >= 500
        assert len(set(ref["elem"][ref["ties"]].tolist())) == 1
        for tol, ulp in WALKS:
            elem, t, _, _, _ = B.walk(b, o, d, tol=tol, rcp_ulp=ulp)
            assert (elem == ref["elem"]).all() and (bits(t) == bits(ref["t"])).all(), (name, tol, ulp)
        elem, t, _, _, _ = B.walk(b, o, d, list_order=False)
        assert (bits(t) == bits(ref["t"])).all()
        wrong[name] = int((elem != ref["elem"]).sum())
    print("rays a walk without the list-order rule gets wrong:", wrong, flush=True)
    assert wrong["s7+g"] >= 500


def test_in_domain_is_the_kernels_test():
    E = 41.0
    lim = 4.0 * E
    u = np.array([0.0, 0.0, 1.0])
    out = np.nextafter(lim, np.inf)
    assert B.in_domain(np.array([lim, -lim, lim]), u, E) and not B.in_domain(np.array([0.0, out, 0.0]), u, E)
    assert not B.in_domain(np.array([-out, 0.0, 0.0]), u, E)
    for bad in (np.nan, np.inf, -np.inf):
        assert not B.in_domain(np.array([bad, 0.0, 0.0]), u, E) and not B.in_domain(np.zeros(3), np.array([0.0, bad, 1.0]), E)
    assert B.in_domain(np.zeros(3), u * (1 + 2.0 ** -22), E) and B.in_domain(np.zeros(3), u * (1 - 2.0 ** -22), E)
    assert not B.in_domain(np.zeros(3), u * 1.000001, E) and not B.in_domain(np.zeros(3), np.zeros(3), E)
    o = np.zeros((130, 3))
    d = np.tile(u, (130, 1))
    d[70] *= 2.0
    assert B.walking_waves(o, d, 130, E).tolist() == [0, 2] and B.walking_waves(o, d, 64, E).tolist() == [0]
    assert B.walking_waves(o, d, 70, E).tolist() == [0, 1] and B.walking_waves(np.zeros(3), d, 130, E).tolist() == [0, 2]


# ---- the population of the batches ---------------------------------------------------------------
@pytest.mark.parametrize("name", BB.LAYOUT_SCENES + BB.HOSTILE_SCENES)
def test_batch_1_holds_what_it_is_chosen_for(name):
    o, d, ref, kind = BB.inside4E(name)
    n = BB.N_RAYS
    assert n == 2597 and o.shape == d.shape == (n, 3)
    E = B.domain_E(name)
    assert B.in_domain(o, d, E).all() and len(B.walking_waves(o, d, n, E)) == 41
    assert min(np.bincount(kind, minlength=4)) >= n // 8
    cube = kind == BB.IN_CUBE
    lo, hi = Q.scene_box(Q.elems_of(name))
    assert ((o[cube] < lo) | (o[cube] > hi)).any(axis=1).mean() > 0.5 and np.abs(o[cube]).max() > 3.5 * E
    hit = ref["elem"] >= 0
    print(name, "hit share %.3f" % hit.mean(), flush=True)
    assert 0.1 <= hit.mean() <= (0.99 if name == "big_flat" else 0.95), hit.mean()
    if name == "big_flat":
        per_kind = np.bincount(kinds_of(name)[ref["elem"][hit]], minlength=6)
        assert min(per_kind[k] for k in Q.OBJECTS) >= 50, per_kind


@pytest.mark.parametrize("name", BB.LAYOUT_SCENES + ("lattice",))
def test_batch_2_holds_what_it_is_chosen_for(name):
    o, d, ref, edits = BB.edge(name)
    E = B.domain_E(name)
    lim = 4.0 * E
    ind = B.in_domain(o, d, E)
    walking = set(B.walking_waves(o, d, len(d), E).tolist())
    for what in (BB.O_IN, BB.D_IN):
        waves = set((np.flatnonzero(edits == what) // 64).tolist())
        assert len(waves & walking) >= 2, BB.EDITS[what]
        assert ind[edits == what].all()
    for what in (BB.O_OUT, BB.D_OUT):
        waves = set((np.flatnonzero(edits == what) // 64).tolist())
        one = [w for w in waves if (~ind[w * 64:w * 64 + 64]).sum() == 1]
        assert len(one) >= 2 and not set(one) & walking, BB.EDITS[what]
        assert not ind[edits == what].any()
    assert (np.abs(o[edits == BB.O_IN]) == lim).any(axis=1).all()
    assert (np.abs(o[edits == BB.O_OUT]).max(axis=1) == np.nextafter(lim, np.inf)).all()
    dd = (d * d).sum(axis=1) - 1
    assert (np.abs(dd[edits == BB.D_IN]) > 2.0 ** -20 * (1 - 2.0 ** -9)).all() and (dd[edits == BB.D_IN] > 0).any() \
        and (dd[edits == BB.D_IN] < 0).any()
    assert (np.abs(dd[edits == BB.D_OUT]) < 2.0 ** -20 * (1 + 2.0 ** -9)).all()
    assert ind[edits == BB.PLAIN].all()
    hit = ref["elem"] >= 0
    assert hit[edits != BB.PLAIN].mean() >= 0.1 and hit[edits == BB.O_IN].mean() >= 0.1 and hit[edits == BB.D_IN].mean() >= 0.1
    # waves that walk and hit a sphere: what a walk that finds nothing gets wrong, and nothing else
    assert len([w for w in walking if hit[w * 64:w * 64 + 64].any()]) >= 20


def test_batch_3_holds_what_it_is_chosen_for():
    o, d, ref, ax, sg, aim = BB.axis()
    E = B.domain_E("lattice")
    assert E == 24.0 and B.in_domain(o, d, E).all() and len(B.walking_waves(o, d, len(d), E)) == 41
    assert ((d * d).sum(axis=1) == 1.0).all()
    rows = np.arange(len(d))
    assert (d[rows, ax] == sg).all() and (o[rows, ax] == -sg * 4.0 * E).all()
    for a in range(3):
        for s in (-1.0, 1.0):
            assert ((ax == a) & (sg == s)).sum() >= 300
        other = np.delete(d[ax == a], a, axis=1)
        assert (np.abs(other) < 1e-30).all()
        assert {"%r" % v for v in other.ravel().tolist()} == {"0.0", "-0.0", "1e-31", "-1e-40"}
    hit = ref["elem"] >= 0
    assert hit.mean() >= 0.25
    assert ((aim == BB.TANGENT) & ~hit).sum() >= 30 and not ((aim == BB.TANGENT) & hit).any()
    assert hit[aim == BB.CENTRE].all() and hit[aim == BB.INSIDE].all() and not hit[aim == BB.OUTSIDE].any()


def test_shadow_batches_hold_what_they_are_chosen_for():
    L, H, E, lit = BB.shadows_s2000()
    assert 2000 <= len(lit) <= 3000 and 0.1 <= lit.mean() <= 0.9 and len({tuple(x) for x in L.tolist()}) == 4
    L, H, E, lit, parts = BB.shadows_l190()
    assert len(parts) == 190 and len(lit) == 190 * 16 and 0.1 <= lit.mean() <= 0.9
    assert len({tuple(x) for x in L.tolist()}) == 190
    L, H, E, lit, by_index = BB.shadows_twins160()
    tw = BB.twin_elements()
    el = Q.elems_of("s160+g")
    assert bytes(el[tw[0]].u) == bytes(el[tw[2]].u) != bytes(el[tw[1]].u)
    assert len(set(Q.canon_roots(el)[i] for i in tw)) == 3, "2 and 2.0 became the same term"
    assert len(lit) >= 64 and 0.1 <= lit.mean() <= 0.9 and all((E == e).sum() >= 8 for e in tw)
    assert (lit == by_index).all() and not lit[E != tw[0]].any()
    # the entries lit only because two elements are the same term: the twins scene (forced onto the BVH
    # by RT_BVH_MIN=2 in tests/test_gpu_query_bvh.py::test_tiny_trees)
    _, _, _, lit2, by_index2 = Q.duplicate_shadows()
    assert ((lit2 == 1) & (by_index2 == 0)).sum() >= 1

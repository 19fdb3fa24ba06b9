"""tests/dispatch_matrix.py against the kernels rt_render.hip really compiles, without a GPU: every
instantiation is classified exactly once; the general-power scenes of the matrix are not vacuous (pow
matters in chains of every length they claim); and the colour bound does what it says."""
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from eraytracer_amd import _native as N
from tests import dispatch_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

FAMILIES = {"k_walk": 60, "k_reflect_shade": 52, "k_render": 32, "k_light": 12, "k_eval_math": 7, "k_walk_deep": 6,
            "k_primary": 4, "k_reflect": 4, "k_pmask": 2, "k_accum": 2, "k_items": 1, "k_selftest_math": 1}


@pytest.fixture(scope="module")
def stubs(tmp_path_factory):
    """The kernel instantiations of rt_render.hip: the __device_stub__ symbols of a host-only compile
    (no device code is generated and no assembly is read), spelled as nm -C spells them, without the
    argument list."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    obj = str(tmp_path_factory.mktemp("stubs") / "rt_render.o")
    src = os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_render.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950:xnack-", "-O1", "-std=c++17", "--cuda-host-only", "-c", src, "-o", obj],
                   check=True, capture_output=True, text=True)
    out = subprocess.run(["nm", "-C", obj], check=True, capture_output=True, text=True).stdout
    names = []
    for line in out.splitlines():
        m = re.search(r"__device_stub__(k_\w+(?:<[^>]*>)?)\(", line)
        if m:
            names.append(m.group(1))
    assert len(names) == len(set(names))
    return sorted(names)


def test_every_instantiation_is_classified_exactly_once(stubs):
    assert Counter(s.split("<")[0] for s in stubs) == FAMILIES and len(stubs) == 183
    table = M.table()
    unclassified = [s for s in stubs if s not in table]
    assert not unclassified, f"kernels nobody says are tested: {unclassified}"
    stale = sorted(set(table) - set(stubs))
    assert not stale, f"classified, but not compiled: {stale}"
    twice = {k: v for k, v in table.items() if len(v) != 1}
    assert not twice, f"classified more than once: {twice}"
    kinds = Counter(v[0][0] for v in table.values())
    print(dict(kinds))
    # rt_eval_math's and rt_selftest_math's kernels have their own tests; the matrix runs every other
    # one: no compiled instantiation is unclassified or unreachable
    assert kinds == {"case": 175, "elsewhere": 8}
    assert all(v[0][0] in ("case", "elsewhere") for v in table.values()) and set(stubs) == set(table)


def test_every_case_claims_something_and_names_are_unique():
    names = [c.name for c in M.CASES]
    assert len(names) == len(set(names))
    for case in M.CASES:
        assert case.child in M.ENV and case.frames
        assert sum(len(M.claims(case, p, g)) for _, p, g in M.instances(case)) > 0, f"{case.name} claims nothing"
        for f in case.frames:
            assert f.w <= 128 and f.h <= 96 and f.base in M.BASES


def test_record_spelling_matches_the_stubs(stubs):
    """rt_debug_launched spells a record from LaunchRecord::spec (rt_render.hip): the family names and
    argument kinds there must be the stubs' (a family whose template changed fails here, on the CPU)."""
    src = open(os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_render.hip")).read()
    spec = re.findall(r'\{"(k_\w+)", (\d), \{([-\d, ]*)\}\}', src)
    assert len(spec) == 10
    spelled = set()
    for name, nargs, radix in spec:
        radix = [int(r) for r in radix.split(",") if r.strip()]
        assert len(radix) == int(nargs)
        kinds = [("false", "true") if r == -2 else tuple(str(i) for i in range(r)) for r in radix]
        for args in ([()] if not radix else __import__("itertools").product(*kinds)):
            spelled.add(name + (f"<{', '.join(args)}>" if radix else ""))
    render = {s for s in stubs if not s.startswith(("k_eval_math", "k_selftest_math"))}
    assert render <= spelled, sorted(render - spelled)
    # what the spec can spell and the compiler did not instantiate: k_walk's and k_reflect_shade's
    # combinations the dispatch code never names
    assert all(s.startswith(("k_walk<", "k_reflect_shade<")) for s in spelled - render)


def test_scenes_take_the_kernels_the_table_says():
    """The power rewrites: 'int' scenes have powers 0 and 1 only, 'gen' scenes a power outside the
    integers 0..1024, and the recipe is the issue's (S64's first sphere powers)."""
    for base in M.BASES:
        for powers, want_int in (("int", True), ("gen", False), ("alt", True)):
            pw = [t[-1][2] for t in M.scene(base, powers) if t[0] in ("sphere", "triangle", "plane")]
            is_int = all(0 <= x <= 1024 and x == int(x) for x in pw)
            if base in ("mixed", "mixed_int", "mixedl40", "default") and powers == "alt":
                assert is_int, base
            else:
                assert is_int == want_int, (base, powers)
        assert len(M.scene(base, "gen")) == len(M.scene(base, "int"))
    assert M.n_lights(M.scene("mixedl40", "gen")) == 40 and M.n_lights(M.scene("s20l33", "gen")) == 33
    rng = M.scenes.SplitMix64(0xA5A5)
    want = [M.P[rng.next_u64() % 7] for _ in range(64)]
    assert [t[3][2] for t in M.scene("s64", "gen") if t[0] == "sphere"] == want
    assert {0.5, 2.5, 1025, 0, 1, 4, 20} == set(want)


@pytest.mark.parametrize("base,w,h,depth,spp", M.general_frames(), ids=lambda v: str(v))
def test_general_power_frames_are_not_vacuous(oracle, base, w, h, depth, spp):
    """The launch record proves that a GENPOW kernel ran; this proves that pow mattered: among the
    pixels with a reflection chain of length n, for every n from 1 to min(depth, 4), at least 5 change
    their oracle colour when the general powers are replaced by integers (P by P_INTEGER)."""
    kw = dict(mode=oracle.MEMO, levels=True, spp=spp, seed=M.SPP_SEED)
    gen, lv = oracle.render(N.marshal(M.scene(base, "gen")), w, h, depth, **kw)
    alt, alv = oracle.render(N.marshal(M.scene(base, "alt")), w, h, depth, **kw)
    assert np.array_equal(lv, alv)
    changed = (gen != alt).any(axis=-1)
    counts = [int((changed & (lv == n)).sum()) for n in range(1, min(depth, 4) + 1)]
    print(base, w, h, depth, spp, counts)
    assert min(counts) >= 5, counts


def test_colour_bound():
    assert M.colour_bound(4, 5) == 2.0 ** -52 * 92 and M.colour_bound(40, 4) == 2.0 ** -52 * 362
    ref = np.array([[1.0, 3.0e4, 0.0], [0.5, 2.0 ** -30, -0.0]])
    ulp = np.spacing(ref)
    worst, bad = M.colour_excess(ref, ref, 4, 5)
    assert (worst, bad) == (0.0, 0)
    # 45 ulps of a value just above a power of two are within 92 x 2^-52 relative; 93 ulps are not
    near = ref + 45 * ulp
    near[ref == 0] = 0.0
    worst, bad = M.colour_excess(near, ref, 4, 5)
    assert bad == 0 and 45 * 0.5 <= worst <= 45 * 1.0001
    far = ref.copy()
    far[0, 0] = 1.0 + 93 * 2.0 ** -52
    assert M.colour_excess(far, ref, 4, 5)[1] == 1
    # the error is measured against the larger of the two, and a wrong light term (1e-9) is caught
    assert M.colour_excess(ref * (1 + 1e-9), ref, 40, 8)[1] == 4
    # where the oracle says +-0 the frame must say 0, however small the difference
    tiny = ref.copy()
    tiny[0, 2] = 2.0 ** -1074
    assert M.colour_excess(tiny, ref, 40, 8)[1] == 1
    tiny[0, 2], tiny[1, 2] = -0.0, 0.0
    assert M.colour_excess(tiny, ref, 4, 5)[1] == 0
    # a NaN is outside every bound
    nan = ref.copy()
    nan[1, 0] = np.nan
    assert M.colour_excess(nan, ref, 4, 5)[1] == 1

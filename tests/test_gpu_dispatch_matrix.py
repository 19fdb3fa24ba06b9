"""Every render-kernel instantiation of rt_render.hip, run and compared (tests/dispatch_matrix.py).

Each case of the matrix is rendered four times (binary64 and binary32 frames, integer and general
specular powers) in a child process (RT_ENGINE, RT_BVH_MIN and RT_BVH_LEVEL are read once per
process), one child per environment and scene class.  The child compares every frame

* bit for bit with the frame of a fresh context with RT_CFG_CULL = 0 and side streams on: brute force
  on the SPH 0 kernels, with the same device pow, so equality is exact with general powers too; a
  binary32 frame equals that binary64 frame rounded; levels, where requested, are equal;
* bit for bit with the other engine's frame, where both engines render it (test_fused_engine);
* with the oracle: the levels equal in every pixel, the colours within 1e-5 and, with powers 0 and 1,
  without a differing bit; with general powers within dispatch_matrix.colour_bound, relative, and
  exactly 0 where the oracle's are (RT_ORDER_FAST sums the same non-negative terms in another order:
  the same bound, with either kind of power);

and reports the launch record of the case's contexts.  The parent asserts that the record holds every
instantiation the table claims for that rendering: the table is checked case by case.

Largest |gpu - oracle| / max(|gpu|, |oracle|) of the general-power frames, in units of 2^-52, as
measured on an MI355X: see DESIGN.md section 3.
"""
import json
import os
import subprocess
import sys

import pytest

from tests import dispatch_matrix as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(tmp_path, env, instances, tag="job", save=None, other=None):
    """Render `instances` ([case name, prec, powers]) in a child with `env`; returns the reports by instance."""
    job = str(tmp_path / f"{tag}.json")
    with open(job, "w") as fh:
        json.dump({"instances": instances, "save": save, "other": other}, fh)
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    r = subprocess.run([sys.executable, "-c", "import sys; from tests import dispatch_matrix as M; M.child_main(sys.argv[1])",
                        job], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "matrix ok" in r.stdout.split("\n"), r.stdout[-4000:] + r.stderr[-4000:]
    reports = [json.loads(line[len("RECORD "):]) for line in r.stdout.splitlines() if line.startswith("RECORD ")]
    assert [[x["case"], x["prec"], x["powers"]] for x in reports] == instances
    return reports


def _instances(cases):
    """The renderings of `cases` that own an instantiation."""
    return [[c.name, p, g] for c in cases for _, p, g in M.instances(c) if M.claims(c, p, g)]


def _check_records(reports):
    for rep in reports:
        case = next(c for c in M.CASES if c.name == rep["case"])
        want = M.claims(case, rep["prec"], rep["powers"])
        assert set(rep["record"]) <= set(M.table()), sorted(set(rep["record"]) - set(M.table()))  # (the spelling)
        missing = sorted(set(want) - set(rep["record"]))
        assert not missing, (f"{rep['case']} prec {rep['prec']} {rep['powers']}: the table claims {missing}, "
                             f"the case launched {rep['record']}")
        # and no rendering ran a kernel of the other pow: GENPOW is the scene's, not the launch's
        other = ", false" if rep["powers"] == "gen" else ", true"
        stray = [k for k in rep["record"] if k.startswith(("k_light<", "k_walk<", "k_reflect_shade<"))
                 and k.split(",")[1] == other[1:]]
        assert not stray, (rep["case"], rep["powers"], stray)


def _group(child, prefix):
    return [c for c in M.CASES if c.child == child and c.name.startswith(prefix)]


# one child per environment and scene class
WAVE_GROUPS = [("wave", "sph2"), ("wave", "wave-common"), ("wave", "sph1"), ("wave", "sph0"), ("bvh", "sph")]


@pytest.mark.parametrize("child,prefix", WAVE_GROUPS)
def test_wavefront_engine(tmp_path, child, prefix):
    cases = _group(child, prefix)
    assert cases
    _check_records(_child(tmp_path, M.ENV[child], _instances(cases)))


def test_fused_engine(tmp_path):
    """RT_ENGINE=fused on S64 (wave beams) and the default scene (none), both orders, levels on and off;
    the frames in the reference's order equal the wavefront engine's, rendered by a child of its own."""
    cases = _group("fused", "fused")
    inst = _instances(cases)
    assert len(cases) == 2 and len(inst) == 8
    wave = str(tmp_path / "wave.npz")
    _child(tmp_path, M.ENV["wave"], inst, tag="wave", save=wave)
    _check_records(_child(tmp_path, M.ENV["fused"], inst, tag="fused", other=wave))


def test_the_cases_cover_the_table():
    """Together the tests above render every case instance that owns an instantiation."""
    ran = {c.name for child, prefix in WAVE_GROUPS + [("fused", "fused")] for c in _group(child, prefix)}
    assert ran == {c.name for c in M.CASES}


def test_launch_record_entry():
    """rt_debug_launched itself: the size it asks for, a cut buffer, the reset and the bad arguments."""
    import ctypes

    import torch

    from eraytracer_amd import _native as N
    L = N.lib()
    el = N.marshal(M.scene("s64", "int"))
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    try:
        assert L.rt_debug_launched(p, None, 0, 0) == 1 and N.launched(p) == frozenset()
        img = torch.zeros((32, 32, 3), dtype=torch.float64, device="cuda")
        N.check(L.rt_launch(p, 32, 32, 3, 16, 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, img.data_ptr(), None,
                            torch.cuda.current_stream().cuda_stream), "rt_launch")
        torch.cuda.synchronize()
        need = L.rt_debug_launched(p, None, 0, 0)
        full = ctypes.create_string_buffer(need)
        assert L.rt_debug_launched(p, full, need, 0) == need and len(full.value) == need - 1
        lines = full.value.decode().splitlines()
        assert full.value.endswith(b"\n") and len(lines) == len(set(lines)) >= 3
        assert set(lines) <= set(M.table()) and "k_items" in lines and "k_primary<0, false>" in lines
        cut = ctypes.create_string_buffer(b"#" * 15, 16)
        assert L.rt_debug_launched(p, cut, 10, 0) == need
        assert cut.raw[:10] == full.value[:9] + b"\0" and cut.raw[10:15] == b"#" * 5
        assert L.rt_debug_launched(None, full, need, 0) == N.RT_EBADARG
        assert L.rt_debug_launched(p, full, -1, 0) == N.RT_EBADARG
        assert L.rt_debug_launched(p, None, 4, 0) == N.RT_EBADARG
        assert N.launched(p, reset=True) == frozenset(lines)
        assert L.rt_debug_launched(p, full, need, 0) == 1 and full.value == b""
    finally:
        L.rt_release(p)

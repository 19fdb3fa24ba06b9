"""Where the LDS-staged tables of a spheres-only scene lie (rt_layout.h's stage_lds_place, called by the
scene compiler for the one-or-sixteen-cells decision and for the header's l_* offsets; read by
stage_tables, rt_cull.inc), without a GPU.

tests/csrc/stage_lds_check.cpp, built with the host sanitizers, sweeps 1..600 spheres x 1..9 lights x
{1, 16} occluder cells and checks every placement against a literal restatement: offsets that are
multiples of 16, ascending, each section at least as long as the bytes stage_tables copies into it,
l_bytes the end of the last, nothing set beyond 32 KiB or with 16 cells, and the returned total for
both cell counts.  The number of staged layouts is restated here.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up16(v):
    return (v + 15) // 16 * 16


def total(n_sph, n_light):
    """Bytes of the six sections with one occluder cell."""
    off = 0
    for size in (96 * n_sph, 16 * n_sph, 32 * n_light * n_sph, 8 * n_light * n_sph * ((n_sph + 63) // 64), 4 * n_sph,
                 32 * n_sph):
        off = up16(off + size)
    return off


def test_placement(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "stage_lds_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "stage_lds_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    cases, staged, unstaged = map(int, r.stdout.split())
    print(f"{cases} cases, one cell: {staged} staged, {unstaged} not staged")
    fits = sum(total(s, l) <= 32 * 1024 for s in range(1, 601) for l in range(1, 10))
    assert cases == 600 * 9 * 2 and (staged, unstaged) == (fits, 600 * 9 - fits)
    assert staged > 0 and unstaged > 0  # both outcomes were seen
    assert total(64, 4) == 19712  # S64: staged

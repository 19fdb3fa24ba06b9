"""Where a launch that walks the sphere BVH keeps it in its dynamic LDS (rt_layout.h's bvh_lds_place,
used by wave_plan for the reflection kernels and by rt_query_launch), without a GPU.

The rule: 64-byte nodes and 32-byte sphere rows are staged, in that order from the base offset, when
together they fit 40 KiB, and not at all otherwise (both offsets -1); every lane's stack follows,
block * bvh_depth 4-byte words — the region scan_bvh indexes by wave and lane.  That is restated here
in three lines and compared with tests/csrc/bvh_lds_check.cpp, built with the host sanitizers.
"""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eraytracer_amd", "csrc")
# (n_bvh, n_sph, bvh_depth): S256, and the staging threshold tests/test_query_bvh.py pins (427 staged, 428 not)
SHAPES = [(255, 256, 10), (426, 427, 11), (427, 428, 11)]
BASES = [0, 21744]  # rt_query_launch's, and behind staged tables (a multiple of 16)


def block_of(unit, name):
    with open(os.path.join(CSRC, unit)) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("bvh_lds") / "bvh_lds_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "bvh_lds_check.cpp"), "-o", out], check=True)
    return out


def restate(n_bvh, n_sph, depth, base, block):
    fits = 64 * n_bvh + 32 * n_sph <= 40 * 1024
    stack = base + (64 * n_bvh + 32 * n_sph if fits else 0)
    return (base if fits else -1, base + 64 * n_bvh if fits else -1, stack, stack + 4 * block * depth)


def test_placement(exe):
    blocks = sorted({256, block_of("rt_render.hip", "BLOCK"), block_of("rt_query.hip", "QUERY_BLOCK")})
    staged = []
    for (n_bvh, n_sph, depth), base, block in itertools.product(SHAPES, BASES, blocks):
        assert base % 16 == 0
        r = subprocess.run([exe, *map(str, (n_bvh, n_sph, depth, base, block))], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        got = tuple(map(int, r.stdout.split()))
        assert got == restate(n_bvh, n_sph, depth, base, block), (n_bvh, n_sph, depth, base, block)
        l_bvh, l_bsph, l_stack, total = got
        # the regions in order from the base, none overlapping, and the stack holds block * depth words
        assert total - l_stack == 4 * block * depth and l_stack % 16 == 0
        assert (l_bvh, l_bsph) == (-1, -1) and l_stack == base or base == l_bvh < l_bsph < l_stack
        staged.append(l_bvh >= 0)
    assert staged == [True] * (2 * len(BASES) * len(blocks)) + [False] * (len(BASES) * len(blocks))

"""The list of active tiles k_pmask leaves beside its masks (rt_plist.h: the buffer's layout, computed
on the host, and the list by its definition), without a GPU.

k_pmask sets a half-tile's flag byte to 1 when every candidate mask of the half-tile is zero
(pe[hw] = any == 0, half-tile hw = 2 * tile + half).  A tile is active when either flag is 0.  The
list holds every active tile once, tile rows in order, with rowoff[r] = the active tiles before tile
row r, so the tiles of tile rows [r0, r1) — a row pass — are list[rowoff[r0] .. rowoff[r1]).  That
is restated here in plain Python for three small geometries and compared with tests/csrc/plist_check.cpp,
built with the host sanitizers around a buffer of exactly the layout's size.
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (W, slab rows, 64-sphere chunks): a partial last tile column and row with an odd number of tile
# rows; one tile; more than 64 tiles per tile row (k_pmask's waves take two steps) and 3 chunks
GEOMS = [(52, 40, 1), (16, 16, 2), (1100, 70, 3)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("plist") / "plist_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "plist_check.cpp"), "-o", out], check=True)
    return out


def restate(w, rows, flags):
    """(rowoff, list) from the flag bytes, by the definition."""
    tiles_x, tile_rows = -(-w // 16), -(-rows // 16)
    rowoff, lst = [], []
    for r in range(tile_rows):
        rowoff.append(len(lst))
        for c in range(tiles_x):
            f0, f1 = flags[2 * (r * tiles_x + c)], flags[2 * (r * tiles_x + c) + 1]
            if not (f0 and f1):
                lst.append((c | f0 << 30 | f1 << 31, r))
    return rowoff + [len(lst)], lst


def patterns(nhalf, seed):
    rnd = random.Random(seed)
    yield [1] * nhalf                                   # no active tile
    yield [0] * nhalf                                   # every tile active, no half empty
    yield [1] * (nhalf - 1) + [0]                       # one active tile, the last, with one empty half
    yield [0, 1] + [1] * (nhalf - 2)                    # one active tile, the first
    yield [int(rnd.random() < 0.7) for _ in range(nhalf)]
    yield [int(rnd.random() < 0.2) for _ in range(nhalf)]


@pytest.mark.parametrize("w,rows,n_chunk", GEOMS)
def test_layout_and_list(exe, w, rows, n_chunk):
    tiles_x, tile_rows = -(-w // 16), -(-rows // 16)
    nhalf = 2 * tiles_x * tile_rows
    for flags in patterns(nhalf, w * 1000 + rows):
        r = subprocess.run([exe, str(w), str(rows), str(n_chunk), "".join(map(str, flags))], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        head, offs, words = r.stdout.splitlines()
        tx, tr, nh, flags_off, rowoff_off, list_off, nbytes = map(int, head.split())
        assert (tx, tr, nh) == (tiles_x, tile_rows, nhalf)
        # the regions in order, none overlapping: masks, flag bytes, tile_rows + 1 offsets, a slot per tile
        assert flags_off == nhalf * n_chunk * 8
        assert rowoff_off >= flags_off + nhalf and rowoff_off % 8 == 0
        assert list_off >= rowoff_off + 4 * (tile_rows + 1) and list_off % 8 == 0
        assert nbytes >= list_off + 8 * tiles_x * tile_rows
        assert nbytes - (nhalf * n_chunk * 8 + nhalf) <= 8 * (tiles_x * tile_rows + tile_rows) + 32  # and no more
        rowoff, lst = restate(w, rows, flags)
        assert list(map(int, offs.split())) == rowoff
        got = list(map(int, words.split()))
        assert list(zip(got[0::2], got[1::2])) == lst
        # complete and free of duplicates; any range of tile rows is one range of the list
        tiles = [(x & 0x3FFFFFFF, y) for x, y in lst]
        assert len(set(tiles)) == len(tiles)
        assert set(tiles) == {(c, r) for r in range(tile_rows) for c in range(tiles_x)
                              if not (flags[2 * (r * tiles_x + c)] and flags[2 * (r * tiles_x + c) + 1])}
        for r0 in range(tile_rows):
            for r1 in range(r0, tile_rows + 1):
                assert all(r0 <= y < r1 for _, y in tiles[rowoff[r0]:rowoff[r1]])
                assert rowoff[r1] - rowoff[r0] == sum(1 for _, y in tiles if r0 <= y < r1)

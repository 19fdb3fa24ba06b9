"""Progressive supersampling (RT_PROGRESSIVE in include/rt_mi355x.h) on the CPU: the header's
contract, the argument checks of rt_launch_samples and rt_resolve (made before any HIP call and
before the context is read, so no device is needed), and the checks of the Python layer, made before
the library is loaded."""
import os
import re

import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import progressive, raytracer, records
from tests.test_window import BAD_WINDOWS, H, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
A = 0x1000  # a pointer that is never dereferenced
SAMPLES_ARGS = ["p", "width", "height", "depth", "x0", "y0", "win_w", "win_h", "row_block", "shard", "nshards", "spp",
                "seed", "sample_begin", "sample_end", "d_sum", "d_levels", "stream"]
RESOLVE_ARGS = ["d_sum", "n_values", "samples", "out_format", "max_value", "d_out", "d_clamped", "stream"]


def declared_args(src, name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, src)
    assert m, f"the header does not declare {name}"
    return [re.sub(r"\s+", " ", a).strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_contract(native):
    src = open(HEADER).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert declared_args(src, "rt_launch_samples") == SAMPLES_ARGS
    assert declared_args(src, "rt_resolve") == RESOLVE_ARGS
    for name in ("rt_launch_samples", "rt_resolve"):
        assert name in N.EXPORTS and not any(ch.isdigit() for ch in name)
        assert hasattr(native.lib(), name)
    # the contract block stands beside the two it builds on, and states the four guarantees
    assert src.index("/* RT_WINDOW") < src.index("/* RT_SUPERSAMPLING") < src.index("/* RT_PROGRESSIVE")
    block = src[src.index("/* RT_PROGRESSIVE"):src.index("typedef struct rt_stats")]
    for g in ("G1", "G2", "G3", "G4"):
        assert re.search(r"\b%s\b" % g, block), g
    assert native.lib().rt_abi_version() == 5 and N.RT_MAX_SPP == 4096
    assert re.search(r"#define\s+RT_MAX_SPP\s+4096\b", src)


def samples(native, *, p=A, w=W, h=H, win=(0, 0, W, H), rb=16, shard=0, nshards=1, spp=4, begin=0, end=4, d_sum=A):
    return native.lib().rt_launch_samples(p, w, h, 5, *win, rb, shard, nshards, spp, 0x5EED, begin, end, d_sum, None,
                                          None)


def test_launch_samples_argument_checks_need_no_device(native):
    bad, big = N.RT_EBADARG, N.RT_ETOOBIG
    assert samples(native, p=None) == bad
    assert samples(native, d_sum=None) == bad
    assert samples(native, d_sum=0x1004) == bad  # not 8-byte aligned
    # the sample range: empty, reversed, past the frame
    assert samples(native, begin=2, end=2) == bad
    assert samples(native, begin=3, end=2) == bad
    assert samples(native, begin=0, end=5) == bad  # sample_end == spp + 1
    assert samples(native, begin=4, end=5) == bad
    assert samples(native, spp=0, begin=0, end=1) == bad
    assert samples(native, spp=0, begin=0, end=0) == bad
    assert samples(native, spp=N.RT_MAX_SPP + 1, begin=0, end=1) == big
    # sizes and shards: rt_launch_window's
    assert samples(native, w=0, h=0, win=(0, 0, 0, 0)) == N.RT_DONE
    assert samples(native, w=0) == bad and samples(native, h=0) == bad
    assert samples(native, rb=0) == bad and samples(native, nshards=0) == bad
    assert samples(native, shard=1, nshards=1) == bad
    assert samples(native, w=(1 << 20) + 1, win=(0, 0, 8, 8)) == big
    assert samples(native, h=(1 << 20) + 1, win=(0, 0, 8, 8)) == big


@pytest.mark.parametrize("what", sorted(BAD_WINDOWS))
def test_launch_samples_refuses_a_bad_window(native, what):
    assert samples(native, win=BAD_WINDOWS[what]) == N.RT_EBADARG
    # ... exactly as rt_launch_window does
    assert native.lib().rt_launch_window(A, W, H, 5, *BAD_WINDOWS[what], 16, 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, 4,
                                         0x5EED, A, None, None) == N.RT_EBADARG


def resolve(native, *, d_sum=A, n=64, samples=4, fmt=N.RT_OUT_U8, maxv=255, d_out=A, d_clamped=None):
    return native.lib().rt_resolve(d_sum, n, samples, fmt, maxv, d_out, d_clamped, None)


def test_resolve_argument_checks_need_no_device(native):
    bad, big = N.RT_EBADARG, N.RT_ETOOBIG
    assert resolve(native, d_sum=None) == bad and resolve(native, d_out=None) == bad
    assert resolve(native, fmt=4) == bad and resolve(native, fmt=-1) == bad
    assert resolve(native, samples=0) == bad
    assert resolve(native, samples=N.RT_MAX_SPP + 1) == big
    # max_value: read for the integer formats only
    assert resolve(native, maxv=0) == bad and resolve(native, fmt=N.RT_OUT_U16, maxv=0) == bad
    assert resolve(native, maxv=256) == big and resolve(native, fmt=N.RT_OUT_U16, maxv=65536) == big
    for fmt in (N.RT_OUT_F64, N.RT_OUT_F32):
        for maxv in (0, 1 << 20):
            assert resolve(native, fmt=fmt, maxv=maxv, n=0) == N.RT_OK
    # alignment: d_sum to 8, d_out to its element, d_clamped to 8
    assert resolve(native, d_sum=0x1004) == bad
    assert resolve(native, fmt=N.RT_OUT_F64, d_out=0x1004) == bad
    assert resolve(native, fmt=N.RT_OUT_F32, d_out=0x1002) == bad
    assert resolve(native, fmt=N.RT_OUT_U16, maxv=65535, d_out=0x1001) == bad
    assert resolve(native, d_clamped=0x1004) == bad
    # what is allowed, with nothing to do: n_values == 0 launches nothing
    assert resolve(native, n=0) == N.RT_OK
    assert resolve(native, n=0, d_out=0x1001, d_clamped=0x1008) == N.RT_OK  # 8-bit samples start anywhere
    assert resolve(native, n=0, fmt=N.RT_OUT_U16, maxv=65535, d_out=0x1002) == N.RT_OK
    assert resolve(native, n=0, fmt=N.RT_OUT_F32, d_out=0x1004, samples=N.RT_MAX_SPP) == N.RT_OK


def test_batch_ends():
    be = progressive.batch_ends
    assert be(4, 1) == [1, 2, 3, 4]
    assert be(4) == [1, 2, 3, 4]
    assert be(4, (1, 1, 2)) == [1, 2, 4]
    assert be(8, 3) == [3, 6, 8]  # the last batch is cut at spp
    assert be(16, 16) == [16] and be(16, 100) == [16] and be(1, 1) == [1]
    assert be(8, [1, 2]) == [1, 3, 5, 7, 8]  # a short sequence goes on with its last size
    assert be(4, (1, 1, 2, 7, 9)) == [1, 2, 4]  # sizes past the frame are not used
    assert be(16, (1, 1, 2, 4, 8)) == [1, 2, 4, 8, 16]
    assert be(N.RT_MAX_SPP, 4096) == [4096]
    for spp in (0, -1, N.RT_MAX_SPP + 1, 2.0, True, None, "4"):
        with pytest.raises(ValueError):
            be(spp, 1)
    for steps in (0, -1, (), (1, 0), (1, -2), 1.5, (1, 2.0), "ab", None, True, (True,)):
        with pytest.raises(ValueError):
            be(4, steps)


BAD_KW = [dict(spp=0), dict(spp=N.RT_MAX_SPP + 1), dict(spp=2.0), dict(spp=True),
          dict(window=(0, 0, 0, 10)), dict(window=(150, 0, 51, 10)), dict(window=(-1, 0, 10, 10)), dict(window="abcd")]
BAD_RENDER_KW = BAD_KW + [dict(steps=0), dict(steps=-3), dict(steps=(1, 0)), dict(steps=()), dict(steps=1.5),
                          dict(precision="u8", max_value=0), dict(precision="u8", max_value=256),
                          dict(precision="u16", max_value=65536), dict(precision="u8", max_value=2.0),
                          dict(precision="f16")]


def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(N, "lib", boom)


@pytest.mark.parametrize("kw", BAD_RENDER_KW, ids=repr)
def test_render_progressive_refuses_bad_arguments_without_the_library(monkeypatch, kw):
    no_library(monkeypatch)
    kw = dict(dict(spp=4), **kw)
    with pytest.raises(ValueError):  # at the call, not at the first item
        raytracer.render_progressive(W, H, records.scene(), 1, **kw)
    with pytest.raises(ValueError):
        raytracer.render_progressive(W, 0, records.scene(), 1, spp=4)
    with pytest.raises(ValueError):
        raytracer.render_progressive(W, H, records.scene(), -1, spp=4)


@pytest.mark.parametrize("kw", BAD_KW + [dict(nshards=0), dict(shard=1, nshards=1), dict(row_block=0), dict(seed=-1)],
                         ids=repr)
def test_progressive_frame_refuses_bad_arguments_without_the_library(monkeypatch, kw):
    no_library(monkeypatch)
    kw = dict(dict(spp=4), **kw)
    with pytest.raises(ValueError):
        progressive.ProgressiveFrame(records.scene(), W, H, 1, **kw)
    with pytest.raises(ValueError):
        progressive.ProgressiveFrame([], W, H, 1, spp=4)  # a scene the marshalling refuses


def test_good_arguments_reach_the_library(monkeypatch):
    no_library(monkeypatch)
    with pytest.raises(AssertionError, match="the library was loaded"):
        progressive.ProgressiveFrame(records.scene(), W, H, 1, spp=4, window=(37, 21, 83, 59))
    it = raytracer.render_progressive(W, H, records.scene(), 1, spp=4, steps=(1, 1, 2), precision="u16", max_value=65535)
    with pytest.raises(AssertionError, match="the library was loaded"):
        next(it)  # the library is loaded when the first item is asked for
    for precision in ("f64", "f32"):  # max_value is not read for float previews
        raytracer.render_progressive(W, H, None, 1, spp=1, precision=precision, max_value=0)

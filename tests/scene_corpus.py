"""The scenes the scene compiler (eraytracer_amd/csrc/rt_scene.cpp) is run over on the CPU: by
tests/test_host.py under the host sanitizers, and by scripts/scene_compile_diff.py, which compares
every byte two trees' compilers produce.

corpus() maps a name to a scene list.  BAD maps the names of the lists that must not compile to the
code compile_scene returns for them; every other scene compiles.  records(scene) is the file of
rt_elem records the C++ drivers read (tests/csrc/scene_check.cpp, scene_dump.cpp).
"""
from eraytracer_amd import _native as N
from eraytracer_amd import records as R
from eraytracer_amd import scenes, terms

RT_EBADARG = -1
# fov 0: tan(0) = 0, so focal_length/2's F = W / 0 is infinite (Erlang: badarith).  The list without
# a camera fails [Camera|Rest]'s use of Camera#camera.location (raytracer.erl:180, :488).
BAD = {"edge:fov0": RT_EBADARG, "edge:no_camera": RT_EBADARG}


def _scaled(scene, k):
    """Every location, centre and radius of a camera-lights-spheres scene times k."""
    def vec(v):
        return R.vector(v[1] * k, v[2] * k, v[3] * k)
    out = []
    for t in scene:
        if t[0] == "camera":
            t = R.camera(vec(t[1]), t[2], t[3], t[4])
        elif t[0] == "point_light":
            t = R.point_light(t[1], vec(t[2]), t[3])
        elif t[0] == "sphere":
            t = R.sphere(t[1] * k, vec(t[2]), t[3])
        out.append(t)
    return out


def _edges():
    cam = R.scene()[0]
    lights = [t for t in scenes.s64() if t[0] == "point_light"]
    mat = R.material(R.colour(0.5, 0.25, 1), 4, 0.5, 0.25)
    ball = R.sphere(1.5, R.vector(1, 0, 9), mat)
    tri = R.triangle(R.vector(-2, 5, 5), R.vector(4, 5, 10), R.vector(4, -5, 10), mat)
    return {
        "lone_camera": lambda: [cam],
        "lights_only": lambda: [cam] + lights,
        "no_light": lambda: [t for t in scenes.s64() if t[0] != "point_light"],
        # sums of squares overflow: cull_ok = 0, infinite |v| in the cone rows
        "s64_1e200": lambda: _scaled(scenes.s64(), 1e200),
        # |v| = 0 and r = 0 in one cone row
        "point_on_light": lambda: [cam] + lights + [R.sphere(0, lights[0][2], mat), ball],
        # exact duplicates (canon chains) and a term that is no object between objects
        "dups_other": lambda: [cam] + lights + [ball, tri, (terms.Atom("fog"), 40), ball, tri, ball],
        # tan(pi / 2) is finite in binary64 (1.6e16): F is tiny, dz = 0, and the scene compiles
        "fov180": lambda: [R.camera(cam[1], cam[2], 180, cam[4])] + R.scene()[1:],
        "fov0": lambda: [R.camera(cam[1], cam[2], 0, cam[4])] + R.scene()[1:],
        "no_camera": lambda: R.scene()[1:],
    }


def corpus():
    """name -> scene list, in a fixed order."""
    from tests import hostile, hostile_flat
    from tests.test_oracle import TRICKY
    c = {"default": R.scene(), "s64": scenes.s64(), "s256": scenes.s256(), "mixed": scenes.synthetic_mixed()}
    for i, mk in enumerate(TRICKY):
        c[f"tricky{i}"] = mk()
    for name in hostile.NAMES:
        c[f"hostile:{name}"] = hostile.build(name)
    for name in hostile_flat.NAMES:
        c[f"flat:{name}"] = hostile_flat.build(name)
    # below, at (2^24 tests with 4 lights) and above OCC_MAX_TESTS: the last has no occluder masks
    for n, seed in ((2000, 7), (2048, 9), (5000, 11)):
        c[f"synthetic{n}"] = scenes.synthetic_scene(n, seed)
    for name, mk in _edges().items():
        c[f"edge:{name}"] = mk()
    assert set(BAD) <= set(c)
    return c


def records(scene):
    """The scene as the bytes of its rt_elem records.  A list without a camera in front, which
    marshal refuses, is marshalled behind one that is then cut off."""
    if scene and scene[0][0] == "camera":
        return bytes(N.marshal(scene))
    arr = N.marshal([R.scene()[0]] + scene)
    for e in arr:
        e.canon -= 1
    return bytes(arr)[len(bytes(arr)) // len(arr):]

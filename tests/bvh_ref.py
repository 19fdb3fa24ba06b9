"""A CPU restatement of the filter the ray queries' BVH walk is (rt_query.hip's bvh_domain, rt_cull.inc's
bvh_inv, bvh_ray, bvh_slab2 and scan_bvh), over the node table the library's own scene compiler built
(tests/csrc/bvh_dump.cpp runs rtl::compile_scene under AddressSanitizer and UBSan and writes it out).

The restatement keeps the kernel's operation order and number formats: binary32 for the reciprocals,
the slab distances, the tolerance products and tlim, entry distances truncated to bfloat16 in the
stack words, and the reference's binary64 expressions in the leaf test.  Two liberties, both far
inside the 2^-16 tolerance the proof at the top of rt_query.hip leaves: the binary32 fma is
float32(float64(a) * float64(b) + float64(c)) (a double rounding), and v_rcp_f32 is the correctly
rounded reciprocal moved by rcp_ulp in {-1, 0, +1} units in the last place.

walk() steps every ray of a batch at once (numpy arrays with one entry per ray, masked by the rays
still walking); each ray's sequence of visits, leaf tests, pushes and pops is the kernel lane's.
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from eraytracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BVH_LDS_MAX = 40 * 1024   # rt_layout.h
NODE_BYTES, ROW_BYTES = 64, 32


# ---- the dump ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dump_exe():
    """tests/csrc/bvh_dump.cpp built with the host sanitizers (a stand-alone program; nothing preloaded)."""
    if shutil.which("g++") is None:
        raise RuntimeError("no g++")
    d = tempfile.mkdtemp(prefix="bvh_dump_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "bvh_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "csrc", "bvh_dump.cpp"),
                    os.path.join(ROOT, "eraytracer_amd", "csrc", "rt_scene.cpp"), "-o", exe], check=True)
    return exe


def dump_elems(elems, bvh_min=None):
    """The compiled BVH of a marshalled scene as a dict (read-only arrays): n_sph, n_bvh, depth, bvh_ok,
    cull_ok, n_obj, n_tri, n_pl, ext, nodes (n_bvh, 16) float32, links and ids (n_bvh, 2) int32, rows
    (n_sph, 4) float64, elem_of (n_obj,) int32.  bvh_min: RT_BVH_MIN of the run."""
    exe = dump_exe()
    d = os.path.dirname(exe)
    fd, src = tempfile.mkstemp(dir=d, suffix=".bin")
    with os.fdopen(fd, "wb") as f:
        f.write(bytes(elems))
    out = src + ".bvh"
    env = dict(os.environ)
    env.pop("RT_BVH_MIN", None)
    if bvh_min is not None:
        env["RT_BVH_MIN"] = str(bvh_min)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    raw = open(out, "rb").read()
    os.remove(src)
    os.remove(out)
    head = np.frombuffer(raw, dtype=np.int32, count=8)
    b = dict(zip(("n_sph", "n_bvh", "depth", "bvh_ok", "cull_ok", "n_obj", "n_tri", "n_pl"), (int(v) for v in head)))
    b["ext"] = float(np.frombuffer(raw, dtype=np.float64, count=1, offset=32)[0])
    off = 40
    nb, ns = b["n_bvh"], b["n_sph"] if b["bvh_ok"] else 0
    b["nodes"] = np.frombuffer(raw, dtype=np.float32, count=nb * 16, offset=off).reshape(nb, 16)
    ints = np.frombuffer(raw, dtype=np.int32, count=nb * 16, offset=off).reshape(nb, 16)
    b["links"], b["ids"] = ints[:, 12:14], ints[:, 14:16]
    off += nb * NODE_BYTES
    b["rows"] = np.frombuffer(raw, dtype=np.float64, count=ns * 4, offset=off).reshape(ns, 4)
    off += ns * ROW_BYTES
    b["elem_of"] = np.frombuffer(raw, dtype=np.int32, count=b["n_obj"] if b["bvh_ok"] else 0, offset=off)
    assert off + 4 * len(b["elem_of"]) == len(raw)
    return b


@functools.lru_cache(maxsize=None)
def dump(name, bvh_min=None):
    from tests import query_ref as Q
    return dump_elems(Q.elems_of(name), bvh_min)


def scene_ext(elems):
    """SceneHdr::ext restated: the largest |coordinate| of the camera, the lights and the sphere centres,
    and the largest |radius| (tests/test_query_bvh.py compares it with the compiled header's)."""
    ext = 0.0
    for e in elems:
        if e.kind == N.RT_CAMERA:
            v = e.u.camera.location
            vals = (v.x, v.y, v.z)
        elif e.kind == N.RT_POINT_LIGHT:
            v = e.u.point_light.location
            vals = (v.x, v.y, v.z)
        elif e.kind == N.RT_SPHERE:
            v = e.u.sphere.center
            vals = (v.x, v.y, v.z, e.u.sphere.radius)
        else:
            continue
        ext = max([ext] + [abs(x) for x in vals])
    return ext


def domain_E(name):
    """E = hdr.ext + 1 of the proof."""
    from tests import query_ref as Q
    return scene_ext(Q.elems_of(name)) + 1.0


# ---- bvh_domain ----------------------------------------------------------------------------------
def in_domain(o, d, E):
    """rt_query.hip's bvh_domain for rays o, d of shape (n, 3): dd summed left to right in binary64, the
    comparisons as written, so a NaN fails."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    lim = 4.0 * E
    dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore"):
        return ((np.abs(o[..., 0]) <= lim) & (np.abs(o[..., 1]) <= lim) & (np.abs(o[..., 2]) <= lim)
                & (np.abs(dd - 1.0) <= 2.0 ** -20))


def walking_waves(o, d, n, E):
    """The indices of the waves of 64 consecutive rays (of the first n) whose active rays all lie in the
    domain: the waves k_query<.., SCAN_BVH> sends down the walk.  o of shape (3,) is one origin for all."""
    d = np.asarray(d)[:n]
    o = np.asarray(o)
    o = np.broadcast_to(o, d.shape) if o.ndim == 1 else o[:n]
    ok = in_domain(o, d, E)
    return np.array([w for w in range((n + 63) // 64) if ok[w * 64:(w + 1) * 64].all()], dtype=np.int64)


# ---- the walk ------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def rcp32(f, rcp_ulp=0):
    r = (1.0 / f.astype(np.float64)).astype(F32)
    if rcp_ulp:
        r = np.nextafter(r, np.copysign(F32(np.inf), r) if rcp_ulp > 0 else F32(0))
    return r


def bvh_inv(d, rcp_ulp=0):
    f = np.asarray(d, dtype=np.float64).astype(F32)
    f = np.where(np.abs(f) < F32(1.0e-30), np.copysign(F32(1.0e-30), f), f).astype(F32)
    return rcp32(f, rcp_ulp)


def bvh_ray(o, d, rcp_ulp=0):
    """(1 / d, -(o * (1 / d))) per axis, binary32, each of shape (n, 3)."""
    inv = bvh_inv(d, rcp_ulp)
    return inv, -(np.asarray(o, dtype=np.float64).astype(F32) * inv)


def bvh_slab2(inv, no, nd, tlim, tol):
    """Both children's slab tests for rays (inv, no (m, 3)) at nodes nd (m, 16): (h (m, 2), tn (m, 2))."""
    LO, HI = F32(1.0) - F32(tol), F32(1.0) + F32(tol)
    tl, tu = [], []
    for a in range(3):
        ia, na = inv[:, a:a + 1], no[:, a:a + 1]
        tl.append(fma32(nd[:, 2 * a:2 * a + 2], ia, na))
        tu.append(fma32(nd[:, 6 + 2 * a:8 + 2 * a], ia, na))
    zero = F32(0.0)
    tn = np.fmax(np.fmax(np.fmin(tl[0], tu[0]), np.fmin(tl[1], tu[1])), np.fmax(np.fmin(tl[2], tu[2]), zero))
    tx = np.fmin(np.fmin(np.fmax(tl[0], tu[0]), np.fmax(tl[1], tu[1])), np.fmin(np.fmax(tl[2], tu[2]), tlim[:, None]))
    return (tn * LO) <= (tx * HI), tn


def walk(bvh, o, d, tol=2.0 ** -16, rcp_ulp=0, list_order=True):
    """scan_bvh for every ray (o, d of shape (n, 3)) as a walking lane runs it.  Returns (elem, t, the
    most stack entries held, visits, popped entries pruned by tlim), arrays of n: elem the scene list
    index of the nearest sphere (-1: none), t its distance (inf: none).  list_order=False: a walk that lacks
    `nearer`'s rule for equal distances (what the tie batches must tell from the kernel's)."""
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    n = len(d)
    nodes, links, ids, rows = bvh["nodes"], bvh["links"], bvh["ids"], bvh["rows"]
    inv, no = bvh_ray(o, d, rcp_ulp)
    HI = F32(1.0) + F32(tol)
    A4 = 4 * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    bt = np.full(n, np.inf)
    bid = np.full(n, 0x7fffffff, dtype=np.int64)
    tlim = np.full(n, np.inf, dtype=F32)
    node = np.zeros(n, dtype=np.int64)
    sp = np.zeros(n, dtype=np.int64)
    stk = np.zeros((n, bvh["depth"] + 1), dtype=np.uint32)
    top = np.zeros(n, dtype=np.int64)
    visits = np.zeros(n, dtype=np.int64)
    pruned = np.zeros(n, dtype=np.int64)

    def leaf(idx, k, cid):
        """sphere_BC<false> + sph_t + nearer for rays idx on local spheres k with compact ids cid."""
        row = rows[k]
        ocx, ocy, ocz = o[idx, 0] - row[:, 0], o[idx, 1] - row[:, 1], o[idx, 2] - row[:, 2]
        B = 2 * (d[idx, 0] * ocx + d[idx, 1] * ocy + d[idx, 2] * ocz)
        C = ocx * ocx + ocy * ocy + ocz * ocz - row[:, 3]
        disc = B * B - A4[idx] * C
        ok = disc >= 0.001
        with np.errstate(invalid="ignore"):
            t = (-B - np.sqrt(np.where(ok, disc, 1.0))) / 2
        upd = ok & (t >= 0) & ((t < bt[idx]) | ((t == bt[idx]) & (cid < bid[idx]) & list_order))
        j = idx[upd]
        bt[j], bid[j] = t[upd], cid[upd]
        tlim[j] = t[upd].astype(F32) * HI

    while True:
        idx = np.flatnonzero(node >= 0)
        if not len(idx):
            break
        # visit
        visits[idx] += 1
        nd = nodes[node[idx]]
        h, tn = bvh_slab2(inv[idx], no[idx], nd, tlim[idx], tol)
        c = links[node[idx]].astype(np.int64)
        cid = ids[node[idx]].astype(np.int64)
        l0, l1 = h[:, 0] & (c[:, 0] < 0), h[:, 1] & (c[:, 1] < 0)
        h0, h1 = h[:, 0] & ~l0, h[:, 1] & ~l1
        both = h0 & h1
        f0 = tn[:, 0] <= tn[:, 1]
        tf = np.where(f0, tn[:, 1], tn[:, 0]).astype(F32)
        far = np.where(f0, c[:, 1], c[:, 0])
        pb = idx[both]
        assert (sp[pb] < bvh["depth"]).all(), "a push past the kernel's bvh_depth stack words"
        assert (far[both] >= 0).all() and (far[both] < 0x10000).all()
        stk[pb, sp[pb]] = (tf[both].view(np.uint32) & np.uint32(0xffff0000)) | far[both].astype(np.uint32)
        sp[pb] += 1
        top[pb] = np.maximum(top[pb], sp[pb])
        node[idx] = np.where(both, np.where(f0, c[:, 0], c[:, 1]), np.where(h0, c[:, 0], np.where(h1, c[:, 1], -1)))
        # leaves: child 0's first, then child 1's for the rays with two
        first = l0 | l1
        col = np.where(l0, 0, 1)[first]
        ii = idx[first]
        leaf(ii, ~c[first, col], cid[first, col])
        two = l0 & l1
        leaf(idx[two], ~c[two, 1], cid[two, 1])
        # pop
        need = idx[node[idx] < 0]
        while len(need):
            need = need[sp[need] > 0]
            if not len(need):
                break
            sp[need] -= 1
            en = stk[need, sp[need]]
            keep = (en & np.uint32(0xffff0000)).view(F32) <= tlim[need]
            node[need[keep]] = (en[keep] & np.uint32(0xffff)).astype(np.int64)
            pruned[need[~keep]] += 1
            need = need[~keep]
    hit = bid != 0x7fffffff
    elem = np.where(hit, bvh["elem_of"][np.where(hit, bid, 0)], -1).astype(np.int32)
    return elem, bt, top, visits, pruned

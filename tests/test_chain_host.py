"""The chained guide pass on the CPU: vk_raytrace_amd/csrc/pt_chain.h (chain_pixel<TWO>, what pt_render_guides_chain runs per lane) compiled for the host
by tests/cpp/chain_host.cpp and held to independent evidence (DESIGN.md section 5.8 is the definition):

  1. identity      with maxLinks = 0, or where nothing is followable, the planes are bit for bit the first-hit guide pass's (tests/guides_host.py, which
                   tests/test_guides_host.py holds to the oracle)
  2. every walk    of every link record is PT_RAYS_CLOSEST of the query host build (tests/test_query_host.py) on the record's origin, direction and seed
  3. the step      between walks -- class, direction, offset origin -- and the folds of tint and length, restated in np.float32 in the operation order
                   of mirror, bend, unit and offset_ray; for mirror and bend the float64 models of tests/golden/gen_float_kat.py already bound the float32
                   error of those functions (tests/test_float_kat.py), so no tolerance is added here: the restatement is bit for bit
  4. planar mirror the virtual point org + dir * plane2, mirrored in the mirror's plane, lies on the end surface: |sum t - t_mirrored| within a
                   first-order bound of the operation sequence (planar_mirror_bound)
  5. what it buys  ghosting under a camera strafe and blur under the a-trous filter on the mirror's pixels, chain guides against first-hit guides:
                   measured, recorded in tests/golden/chain_kat_tol.json, and guarded against regression
  6. edges         masks, tiny images, refusals, a class turned off, overflow counting
  7. mutations     five planted breaks of pt_chain.h, each failing a named test

The fixture is tests/chain_scenes.py's mirror room; test_the_room_exercises_every_class asserts its census.  tests/test_chain_gpu.py holds the device to
this host build."""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import chain_host as ch, chain_scenes, denoise_host as dh, guides_host, temporal_host as th
from tests import test_guides_host as host
from tests import test_query_host as qhost
from tests.golden.gen_temporal_kat import U, V
from tests.host_harness import CSRC, TracedScene
from vk_raytrace_amd import capi, host_device as hd, synth

SIZES, APERTURES, MISS_DEPTH, bits = host.SIZES, host.APERTURES, host.MISS_DEPTH, host.bits
TOL_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_kat_tol.json")
CENSUS_LINKS = 3          # maxLinks of the census: link counts 0 .. 3 and the link limit all occur
CENSUS_MIN = 20           # pixels each class must occur on at 96 x 64
ROOM = "mirror-room"
ALPHA_SCENES = host.ALPHA_SCENES      # fuzz0, fuzz1, fuzz5, sponza-like


class RoomCase:
    """a scene of tests/chain_scenes.py on the host harness (the cases of tests/test_guides_host.py carry an oracle besides)"""

    def __init__(self, name, scene):
        self.name, self.scene = name, scene
        self.traced = TracedScene(scene)

    def set_camera(self, width, height, aperture):
        cam = host.camera_for(self.scene, width, height, aperture)
        guides_host.set_camera(self.traced, cam)
        return cam


@functools.lru_cache(maxsize=None)
def case(name):
    if name == ROOM:
        return RoomCase(name, chain_scenes.mirror_room())
    if name == "matte-room":
        return RoomCase(name, chain_scenes.matte_room())
    return host.case(name)


SCENES = (ROOM, "matte-room") + tuple(ALPHA_SCENES)


@functools.lru_cache(maxsize=None)
def room_chain(width, height, aperture, two, max_links=CENSUS_LINKS):
    """(planes, link plane, records, counts) of the room; computed once and shared, read-only"""
    c = case(ROOM)
    c.set_camera(width, height, aperture)
    p = ch.params(max_links)
    planes, links = ch.chain(c.traced, two, width, height, p, 7, MISS_DEPTH)
    rec, cnt = ch.links(c.traced, two, width, height, p, miss_depth=MISS_DEPTH)
    for a in planes + (links, rec, cnt):
        a.setflags(write=False)
    return planes, links, rec, cnt


def assert_planes_equal(got, want, what):
    for j in range(3):
        same = (bits(got[j]) == bits(want[j])).all(-1)
        assert same.all(), f"{what}: plane {j} differs at {np.count_nonzero(~same)} pixels, first (y, x) {np.argwhere(~same)[:4].tolist()}"


# ---- 0. the fixture ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_room_exercises_every_class():
    """at 96 x 64, pinhole, maxLinks = 3, on both structures: each end code 0, 1, 2, each class mirror / glass / thin-walled / total internal reflection
    and each link count 0 .. 3 occurs on at least 20 pixels"""
    w, h = SIZES[0]
    for two in (0, 1):
        _, links, rec, cnt = room_chain(w, h, 0.0, two)
        ends, counts = np.bincount((links >> 8).ravel(), minlength=4), np.bincount((links & 255).ravel(), minlength=CENSUS_LINKS + 1)
        assert (ends[:3] >= CENSUS_MIN).all() and (counts[:CENSUS_LINKS + 1] >= CENSUS_MIN).all(), (ends, counts)
        assert len(counts) == CENSUS_LINKS + 1
        valid = np.arange(ch.LINK_SLOTS)[None, :] < cnt[:, None]
        for cls in (ch.MIRROR, ch.GLASS, ch.THIN, ch.TIR):
            n = int(((rec["cls"] == cls) & valid).any(1).sum())
            assert n >= CENSUS_MIN, (cls, n)
        # the records agree with the link plane: one record per followed surface and one for the end surface, none after a miss of the camera ray
        l, e = (links & 255).ravel(), (links >> 8).ravel()
        assert np.array_equal(cnt, np.where(e == ch.END_MISS, l, l + 1))


def test_the_host_builds_of_both_structures_agree_on_the_room_and_fuzz1():
    """flat == two-level on the scenes the device is compared on (tests/test_chain_gpu.py counts on it: the reference alone stays inside its cap)"""
    for name in (ROOM, "fuzz1"):
        c = case(name)
        for (w, h) in SIZES:
            for ap in APERTURES:
                c.set_camera(w, h, ap)
                a = ch.chain(c.traced, 0, w, h, ch.params(8), 7, MISS_DEPTH)
                b = ch.chain(c.traced, 1, w, h, ch.params(8), 7, MISS_DEPTH)
                assert_planes_equal(a[0], b[0], f"{name} {w}x{h} aperture {ap}")
                assert np.array_equal(a[1], b[1])


# ---- 1. identity --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_without_links_the_planes_are_the_first_hit_pass(name):
    c = case(name)
    for (w, h) in SIZES:
        for ap in APERTURES:
            c.set_camera(w, h, ap)
            for two in (0, 1):
                want = guides_host.guides(c.traced, two, w, h, 7, MISS_DEPTH)
                got, links = ch.chain(c.traced, two, w, h, ch.params(0), 7, MISS_DEPTH)
                assert_planes_equal(got, want, f"{name} {w}x{h} aperture {ap} two={two}")
                miss = want[2][..., 0] == np.float32(MISS_DEPTH)
                assert (links & 255 == 0).all() and np.array_equal(links >> 8 == ch.END_MISS, miss) and np.isin(links >> 8, (0, 1, 2)).all()


def test_where_nothing_is_followable_the_planes_are_the_first_hit_pass():
    p, seen = ch.params(8), 0
    for name in SCENES:
        c = case(name)
        if chain_scenes.followable_by_factors(c.scene, p):
            continue
        seen += 1
        for (w, h) in SIZES:
            for ap in APERTURES:
                c.set_camera(w, h, ap)
                for two in (0, 1):
                    want = guides_host.guides(c.traced, two, w, h, 7, MISS_DEPTH)
                    got, links = ch.chain(c.traced, two, w, h, p, 7, MISS_DEPTH)
                    assert_planes_equal(got, want, f"{name} {w}x{h} aperture {ap} two={two}")
                    miss = want[2][..., 0] == np.float32(MISS_DEPTH)
                    assert np.array_equal(links, np.where(miss, np.uint32(1 << 8), np.uint32(0)))
                    assert 0.1 < miss.mean() < 0.9
    assert seen >= 1 and chain_scenes.followable_by_factors(case(ROOM).scene, p)


# ---- 2. every walk is the trace contract's ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (ROOM, "fuzz1"))
def test_every_walk_is_the_query_host_builds_closest_hit(name):
    """(t, instance, primitive) of every link record == PT_RAYS_CLOSEST on the record's origin, direction and seed, bit for bit, on both structures; and
    the seed a record starts from is the seed the query of the previous record leaves (the RNG state runs on through the chain).  On fuzz1 every surface
    is followed (maxRoughness = 1, minMetallic = 0), so that walks after alpha draws exist"""
    c = case(name)
    w, h = SIZES[0] if name == ROOM else SIZES[1]
    p = ch.params(8) if name == ROOM else ch.params(8, 1.0, 0.0, 0.0)
    walks = drew = carried = 0
    for ap in APERTURES:
        c.set_camera(w, h, ap)
        for two in (0, 1):
            rec, cnt = ch.links(c.traced, two, w, h, p, miss_depth=MISS_DEPTH)
            valid = np.arange(ch.LINK_SLOTS)[None, :] < cnt[:, None]
            r = rec[valid]
            hits = qhost.host_query(c.traced, two, qhost.CLOSEST, qhost.make_rays(r["org"], r["dir"], seeds=r["seed"]))
            assert (hits["status"] & qhost.HIT != 0).all()
            assert np.array_equal(bits(hits["t"]), bits(r["t"])) and np.array_equal(hits["instanceID"], r["instance"]) and np.array_equal(hits["primitiveID"].astype(np.uint32), r["primitive"])
            assert np.array_equal(bits(hits["u"]), bits(r["u"])) and np.array_equal(bits(hits["v"]), bits(r["v"]))
            after = np.zeros(rec.shape, np.uint32)
            after[valid] = hits["seed"]
            follows = valid[:, 1:]
            assert np.array_equal(rec["seed"][:, 1:][follows], after[:, :-1][follows])
            walks += len(r)
            drew += int(np.count_nonzero(after[valid] != r["seed"]))
            carried += int(np.count_nonzero(rec["seed"][:, 1:][follows] != np.broadcast_to(rec["seed"][:, :1], follows.shape)[follows]))
    assert walks > 1000
    if name == "fuzz1":
        assert drew > 0 and carried > 0     # (alpha draws of a walk, and later walks that start from a seed they left: the room has no alpha)


# ---- 3. the step between walks --------------------------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mirror32(i, n):
    """pt_math.h mirror: I - N * (2 * dot(N, I))"""
    return i - n * (f32(2.0) * dot3(n, i))[..., None]


def bend32(i, n, eta):
    """pt_math.h bend (GLSL refract): zero when k < 0"""
    d = dot3(n, i)
    k = f32(1.0) - eta * eta * (f32(1.0) - d * d)
    with np.errstate(invalid="ignore"):
        out = i * eta[..., None] - n * (eta * d + np.sqrt(k))[..., None]
    return np.where((k < 0)[..., None], f32(0.0), out).astype(f32)


def unit32(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1.0) / np.sqrt(dot3(a, a))
        return a * inv[..., None]


def offset_ray32(p, n):
    """pt_shade.h offset_ray (Ray Tracing Gems ch. 6)"""
    o = (f32(256.0) * n).astype(np.int32)       # (truncation toward zero, as the C conversion)
    pi = (p.view(np.int32) + np.where(p < 0, -o, o)).view(f32)
    return np.where(np.abs(p) < f32(1.0 / 32.0), p + f32(1.0 / 65536.0) * n, pi).astype(f32)


def restate_step(r, p):
    """(class, new direction, new origin) of link records r (a flat array) under parameters p, in np.float32"""
    rough_ok = r["roughness"] <= f32(p.maxRoughness)
    is_mirror = rough_ok & (r["metallic"] >= f32(p.minMetallic))
    is_glass = rough_ok & ~is_mirror & ((f32(1.0) - r["metallic"]) * r["transmission"] >= f32(p.minTransmission))
    d, n = r["dir"], r["ffnormal"]
    b = bend32(d, n, r["eta"])
    tir = ~b.any(-1)
    refl = mirror32(d, n)
    thin = r["thin"] != 0
    cls = np.where(is_mirror, ch.MIRROR, np.where(is_glass, np.where(thin, ch.THIN, np.where(tir, ch.TIR, ch.GLASS)), ch.END)).astype(np.uint32)
    L = np.where((cls == ch.MIRROR)[:, None] | (cls == ch.TIR)[:, None], refl, np.where((cls == ch.GLASS)[:, None], unit32(b), d)).astype(f32)
    side = np.where((dot3(L, n) > 0)[:, None], n, -n)
    return cls, L, offset_ray32(r["position"], side)


@pytest.mark.parametrize("two", (0, 1))
def test_the_step_between_walks_restated_in_float32(two):
    """class, direction and offset origin of every link record of the room give the next record bit for bit; tint and length folded in float32 in link
    order give planes 0 and 2 bit for bit.  The float32 error of mirror and bend themselves is bounded by gen_float_kat.py's float64 models
    (tests/test_float_kat.py); nothing is added to that here"""
    for (w, h) in SIZES:
        for ap in APERTURES:
            planes, links, rec, cnt = room_chain(w, h, ap, two)
            p = ch.params(CENSUS_LINKS)
            l, e = (links & 255).ravel(), (links >> 8).ravel()
            tint, dist = np.ones((w * h, 3), f32), np.zeros(w * h, f32)
            for k in range(ch.LINK_SLOTS - 1):
                here = cnt > k
                r = rec[here, k]
                cls, L, org = restate_step(r, p)
                followed = l[here] > k
                # a followable surface at the limit is an end (code 2); everything else has the restated class
                limit = ~followed & (e[here] == ch.END_LIMIT)
                assert (cls[limit] != ch.END).all() and (r["cls"][limit] == ch.END).all() and (l[here][limit] == p.maxLinks).all()
                assert np.array_equal(np.where(limit, ch.END, cls), r["cls"]), k
                assert np.array_equal(followed, r["cls"] != ch.END)
                nxt_here = followed & (cnt[here] > k + 1)       # (a walk that leaves the scene has no record)
                nxt = rec[here, k + 1][nxt_here]
                assert np.array_equal(bits(nxt["dir"]), bits(L[nxt_here])) and np.array_equal(bits(nxt["org"]), bits(org[nxt_here])), k
                idx = np.nonzero(here)[0][followed]
                tint[idx] = tint[idx] * r["albedo"][followed]
                dist[idx] = dist[idx] + r["t"][followed]
            on_surface = e != ch.END_MISS
            last = rec[np.arange(w * h), np.maximum(cnt, 1) - 1]
            want0 = np.where(on_surface[:, None], f32(0.0) + tint * last["albedo"], np.where((l > 0)[:, None], f32(0.0) + tint, f32(0.0))).astype(f32)
            want2 = np.where(on_surface, dist + last["t"], np.where(l > 0, dist + f32(MISS_DEPTH), f32(MISS_DEPTH))).astype(f32)
            assert np.array_equal(bits(planes[0][..., :3].reshape(-1, 3)), bits(want0))
            assert np.array_equal(bits(planes[2][..., 0].ravel()), bits(want2)) and not bits(planes[2][..., 1:]).any()
            assert (planes[0][..., 3] == 1).all() and (planes[1][..., 3] == 1).all()
            assert not planes[1][..., :3].reshape(-1, 3)[~on_surface].any()


# ---- 4. planar mirror -------------------------------------------------------------------------------------------------------------------------------------------------
def t2_distance(org, d, tri):
    """t of the trace contract's triangle test T2 (pt_trace.h tri_test) in its operation order, on V values: tri = (p0, e1, e2) as lists of three V"""
    p0, e1, e2 = tri
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]   # noqa: E731
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]                                               # noqa: E731
    pv = cross(d, e2)
    inv = V(np.ones_like(pv[0].v), np.zeros_like(pv[0].v)) / dot(e1, pv)
    tv = [org[i] - p0[i] for i in range(3)]
    u = dot(tv, pv) * inv
    qv = cross(tv, e1)
    v = dot(d, qv) * inv
    return dot(e2, qv) * inv, u, v


def planar_mirror_bound(two=1):
    """Pinhole pixels of the room at 96 x 64 whose chain is camera -> the mirror in x = -MIRROR_X -> end surface.  In exact arithmetic, with the second
    ray starting AT the mirror point P0 = E + D tau0, the ray from the mirrored eye E' = (-2 MIRROR_X - Ex, Ey, Ez) along D' = (-Dx, Dy, Dz) meets the end
    surface at tau0 + tau1: the planar-mirror identity.  What separates sum t = fl(t0 + t1) from the query's t_m, to first order (u = 2^-24):

      e_sum   the running first-order bound of T2's operation sequence for t0 and t1 and of their sum, carried by gen_temporal_kat.V through a float64
              restatement from the float32 inputs (eye, direction, the record's origin, the triangles as the structure holds them);
      e_m     the same for t_m from the float32-rounded mirrored eye, plus that rounding's shift of the origin, u |E'x|, seen along the ray: / c1;
      g       the second ray starts at offset_ray(position), not at P0.  |position - P0| <= e_pos, the running bound of the barycentric interpolation
              from T2's u and v, plus 6 u R for the edges the structure stores rounded and the identity transform (R: the largest coordinate involved);
              offset_ray moves a coordinate by at most 256 float32 steps of it.  A shift s of the origin changes the distance to the end surface's plane
              along L by (s . n1) / (L . n1): g = (e_pos + 6 u R + 256 spacing(R)) / c1, c1 = |L . n1|.

    Returns per pixel (|sum t - t_m|, bound) and the number of pixels looked at / of pixels whose mirrored ray meets another primitive (silhouettes)."""
    w, h = SIZES[0]
    c = case(ROOM)
    planes, links, rec, cnt = room_chain(w, h, 0.0, two)
    first = rec[:, 0]
    sel = (links.ravel() == 1) & (cnt == 2) & (first["cls"] == ch.MIRROR) & (first["ffnormal"] == np.array([1, 0, 0], f32)).all(1) & (first["position"][:, 0] < 0)
    r0, r1 = rec[sel, 0], rec[sel, 1]
    assert sel.sum() > 200
    E, D = r0["org"], r0["dir"]
    assert np.array_equal(bits(r1["dir"]), bits(D * np.array([-1, 1, 1], f32)))     # the mirrored direction, exactly
    Em = E.astype(np.float64) * [-1, 1, 1] + [-2 * chain_scenes.MIRROR_X, 0, 0]
    Em32, Dm = Em.astype(f32), r1["dir"]
    hits = qhost.host_query(c.traced, two, qhost.CLOSEST, qhost.make_rays(Em32, Dm))
    same = (hits["instanceID"] == r1["instance"]) & (hits["primitiveID"].astype(np.uint32) == r1["primitive"])
    tri = lambda refs: [[V(np.array([c.traced.world_tri(int(x))[0][3 * k + i] for x in refs]), np.zeros(len(refs))) for i in range(3)] for k in range(3)]   # noqa: E731
    vec = lambda a: [V(a[:, i].astype(np.float64), np.zeros(len(a))) for i in range(3)]   # noqa: E731
    tri0, tri1 = tri(r0["ref"]), tri(r1["ref"])
    t0, u0, v0 = t2_distance(vec(E), vec(D), tri0)
    t1, _, _ = t2_distance(vec(r1["org"]), vec(Dm), tri1)
    tm, _, _ = t2_distance(vec(Em32), vec(Dm), tri1)
    total = t0 + t1
    # position = p0 b0 + p1 u + p2 v, with p1 = p0 + e1, p2 = p0 + e2
    one = V(np.ones(len(E)), np.zeros(len(E)))
    b0 = one - u0 - v0
    pos = [tri0[0][i] * b0 + (tri0[0][i] + tri0[1][i]) * u0 + (tri0[0][i] + tri0[2][i]) * v0 for i in range(3)]
    e_pos = np.sqrt(sum(p.e ** 2 for p in pos))
    n1 = np.cross(np.stack([x.v for x in tri1[1]], 1), np.stack([x.v for x in tri1[2]], 1))
    c1 = np.abs((Dm.astype(np.float64) * n1).sum(1)) / np.linalg.norm(n1, axis=1)
    R = np.maximum(np.abs(Em).max(1), np.abs(r1["position"]).max(1)).astype(np.float64)
    g = (e_pos + 6 * U * R + 256 * np.spacing(R.astype(f32)).astype(np.float64)) / c1
    bound = total.e + tm.e + U * np.abs(Em[:, 0]) / c1 + g
    sum_t = planes[2][..., 0].ravel()[sel]
    assert np.array_equal(bits(sum_t), bits(r0["t"] + r1["t"]))
    err = np.abs(sum_t.astype(np.float64) - hits["t"].astype(np.float64))
    return err[same], bound[same], int(sel.sum()), int((~same).sum())


def test_a_planar_mirror_gives_the_mirror_image_as_virtual_point():
    """|sum t - t_mirrored| <= planar_mirror_bound on every pixel whose mirrored ray meets the same primitive; at most 2 % of the pixels (silhouettes,
    where the two rays may fall on either side of an edge) meet another one.  The worst ratio is recorded in chain_kat_tol.json"""
    err, bound, n, other = planar_mirror_bound()
    assert other <= 0.02 * n, (other, n)
    ratio = float((err / bound).max())
    print(f"planar mirror: {len(err)} pixels, worst |sum t - t_m| {err.max():.3e}, worst ratio to the bound {ratio:.3f}, {other} silhouette pixels")
    assert ratio <= 1.0, ratio
    assert abs(json.load(open(TOL_PATH))["planar_mirror"]["worst_ratio"] - ratio) < 1e-6


# ---- 5. what it buys ------------------------------------------------------------------------------------------------------------------------------------------------
def guides_at(eye, center, w, h, chained):
    c = case(ROOM)
    cam0 = c.scene.camera
    old = (cam0.eye, cam0.center)
    cam0.eye, cam0.center = eye, center
    try:
        cam = c.set_camera(w, h, 0.0)
        w2c = capi.camera_world_to_clip(cam0, w / h)
        planes, links = ch.chain(c.traced, 0, w, h, ch.params(8 if chained else 0), 7, 100.0)
    finally:
        cam0.eye, cam0.center = old
    return planes, links, cam, w2c


def measure_what_it_buys():
    """{"ghosting": {...}, "blur": {...}}: the errors on the pixels of one mirror link with chain guides and with first-hit guides (see the module
    docstring, 5), on the CPU host builds of the temporal step and of the a-trous filter"""
    w, h = SIZES[0]
    c = case(ROOM)
    eye_a, center_a = c.scene.camera.eye, c.scene.camera.center
    eye_b, center_b = chain_scenes.strafed(c.scene.camera)
    out = {}
    chain_a, links_a, cam_a, w2c_a = guides_at(eye_a, center_a, w, h, True)
    chain_b, links_b, cam_b, w2c_b = guides_at(eye_b, center_b, w, h, True)
    first_a = guides_at(eye_a, center_a, w, h, False)[0]
    first_b = guides_at(eye_b, center_b, w, h, False)[0]
    one_link = (links_a == 1) & (links_b == 1)
    assert one_link.sum() > 300
    colour_a, colour_b = chain_a[0], chain_b[0]       # noise-free, and it shows the reflected checker
    ghost = {}
    for what, (ga, gb) in (("chain", (chain_a, chain_b)), ("first_hit", (first_a, first_b))):
        rc, hist = th.temporal(colour_a, ga[1], ga[2], cam_a.viewInverse, cam_a.projInverse, th.params(w2c_a, 0.05, 0.05, 32.0))
        assert rc == 0
        rc, hist = th.temporal(colour_b, gb[1], gb[2], cam_b.viewInverse, cam_b.projInverse, th.params(w2c_b, 0.05, 0.05, 32.0), hist)
        assert rc == 0
        ghost[what] = float(np.abs(hist.colour[..., :3] - colour_b[..., :3])[one_link].mean())
        ghost[what + "_history_length"] = float(hist.length[one_link].mean())
    ghost["ratio"] = ghost["chain"] / ghost["first_hit"]
    out["ghosting"] = ghost
    rng = np.random.default_rng(7)
    noisy = colour_a.copy()
    noisy[..., :3] += rng.normal(0.0, 0.2, (h, w, 3)).astype(np.float32)
    blur = {}
    for what, g in (("chain", chain_a), ("first_hit", first_a)):
        rc, den = dh.denoise(noisy, g, dh.params(5, 0.0, (0.1, 0.1, 0.1)))
        assert rc == 0
        blur[what] = float(np.abs(den[..., :3] - colour_a[..., :3])[links_a == 1].mean())
    blur["noisy"] = float(np.abs(noisy[..., :3] - colour_a[..., :3])[links_a == 1].mean())
    blur["ratio"] = blur["chain"] / blur["first_hit"]
    out["blur"] = blur
    return out


def test_what_the_chain_buys_is_what_was_recorded():
    """a regression guard against the recorded values, not a target: the chain's error stays below the first-hit error by at least half of the recorded
    margin, for the ghosting under a strafe and for the blur of the a-trous filter"""
    rec, got = json.load(open(TOL_PATH)), measure_what_it_buys()
    for what in ("ghosting", "blur"):
        print(what, got[what])
        recorded = rec[what]["ratio"]
        assert recorded < 1.0
        assert got[what]["ratio"] <= 1.0 - (1.0 - recorded) / 2, (what, got[what], recorded)


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_mask_of_one_plane_writes_only_that_plane():
    c = case(ROOM)
    w, h = SIZES[1]
    c.set_camera(w, h, APERTURES[1])
    full, links = ch.chain(c.traced, 0, w, h, ch.params(8), 7, MISS_DEPTH)
    sentinel = np.float32(-7.25)
    for j in range(3):
        into = [np.full((h, w, 4), sentinel, np.float32) for _ in range(3)]
        got, l = ch.chain(c.traced, 0, w, h, ch.params(8), 1 << j, MISS_DEPTH, into=into)
        assert np.array_equal(l, links)
        for k in range(3):
            if k == j:
                assert np.array_equal(bits(got[k]), bits(full[k])), (j, k)
            else:
                assert (got[k] == sentinel).all(), (j, k)


@pytest.mark.parametrize("size", [(1, 1), (9, 9)])
def test_tiny_images(size):
    """a 1 x 1 and a 9 x 9 image: every pixel is the pixel of the per-pixel records, and the 9 x 9 image follows links"""
    c = case(ROOM)
    w, h = size
    c.set_camera(w, h, 0.0)
    for two in (0, 1):
        planes, links = ch.chain(c.traced, two, w, h, ch.params(8), 7, MISS_DEPTH)
        rec, cnt = ch.links(c.traced, two, w, h, ch.params(8), miss_depth=MISS_DEPTH)
        l, e = (links & 255).ravel(), (links >> 8).ravel()
        assert np.array_equal(cnt, np.where(e == ch.END_MISS, l, l + 1))
        want = guides_host.guides(c.traced, two, w, h, 7, MISS_DEPTH)
        unfollowed = (l == 0)
        for j in range(3):
            assert np.array_equal(bits(planes[j].reshape(-1, 4)[unfollowed]), bits(want[j].reshape(-1, 4)[unfollowed]))
        if size == (9, 9):
            assert (l > 0).any()


def test_every_refusal_has_its_own_text():
    good = dict(max_links=4, max_roughness=0.05, min_metallic=0.9, min_transmission=0.9)
    assert ch.constants(ch.params(**good)) == (capi.PT_OK, "")
    assert ch.constants(ch.params(0, 0.0, 0.0, 0.0))[0] == capi.PT_OK and ch.constants(ch.params(8, 3.0e38, 2.0, 2.0))[0] == capi.PT_OK
    cases = [(None, "null"), (ch.params(**dict(good, max_links=9)), "maxLinks"), (ch.params(**dict(good, max_links=0xFFFFFFFF)), "maxLinks")]
    for field, word in (("max_roughness", "maxRoughness"), ("min_metallic", "minMetallic"), ("min_transmission", "minTransmission")):
        cases += [(ch.params(**dict(good, **{field: v})), word) for v in (-1.0, float("nan"), float("inf"), -0.5e-30)]
    cases += [(ch.params(flags=f, **good), "flag") for f in (1, 0x80000000)]
    reasons = set()
    for p, word in cases:
        rc, why = ch.constants(p)
        assert rc == capi.PT_ERR_INVALID and word in why, (word, why)
        reasons.add(why)
    assert len(reasons) == 6
    assert ch.need_plane(True) == (capi.PT_OK, "")
    rc, why = ch.need_plane(False)
    assert rc == capi.PT_ERR_STATE and "pt_render_guides_chain" in why
    # a refused call writes nothing
    c = case(ROOM)
    c.set_camera(9, 9, 0.0)
    out = np.full((9, 9, 4), 3.5, np.float32)
    links = np.full((9, 9), 77, np.uint32)
    over = C.c_uint32(5)
    p = ch.params(flags=1, **good)
    rc = ch.lib().ch_chain(c.traced.h, 0, 9, 9, C.byref(p), 7, 1.0, out.ctypes.data, out.ctypes.data, out.ctypes.data, links.ctypes.data, C.byref(over))
    assert rc == capi.PT_ERR_INVALID and (out == 3.5).all() and (links == 77).all()


def test_a_threshold_above_one_turns_its_class_off():
    """minMetallic = 2: no mirror is followed, and the result is that of the glass class alone -- the chain of a pixel is the chain with both classes up
    to its first mirror; minTransmission = 2 likewise"""
    w, h = SIZES[0]
    c = case(ROOM)
    c.set_camera(w, h, 0.0)
    both = ch.links(c.traced, 0, w, h, ch.params(8), miss_depth=MISS_DEPTH)
    for off, kw in (((ch.MIRROR,), dict(min_metallic=2.0)), ((ch.GLASS, ch.THIN, ch.TIR), dict(min_transmission=2.0))):
        p = ch.params(8, **kw)
        planes, links = ch.chain(c.traced, 0, w, h, p, 7, MISS_DEPTH)
        rec, cnt = ch.links(c.traced, 0, w, h, p, miss_depth=MISS_DEPTH)
        valid = np.arange(ch.LINK_SLOTS)[None, :] < cnt[:, None]
        assert not (np.isin(rec["cls"], off) & valid).any() and (links & 255).max() > 0
        # the records of the run with both classes, cut at the first surface of the class that is off
        brec, bcnt = both
        is_off = np.isin(brec["cls"], off) & (np.arange(ch.LINK_SLOTS)[None, :] < bcnt[:, None])
        cut = np.where(is_off.any(1), is_off.argmax(1) + 1, bcnt)
        assert np.array_equal(cnt, cut)
        for k in range(ch.LINK_SLOTS):
            here = cnt > k
            a, b = rec[here, k], brec[here, k]
            for f in ("org", "dir", "seed", "t", "instance", "primitive", "albedo"):
                assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (off, k, f)
            ended = cnt[here] == k + 1
            assert np.array_equal(np.where(ended & np.isin(b["cls"], off), ch.END, b["cls"]), a["cls"])
    # both off: the first-hit pass
    c.set_camera(w, h, 0.0)
    planes, links = ch.chain(c.traced, 0, w, h, ch.params(8, min_metallic=2.0, min_transmission=2.0), 7, MISS_DEPTH)
    assert_planes_equal(planes, guides_host.guides(c.traced, 0, w, h, 7, MISS_DEPTH), "both classes off")
    assert (links & 255 == 0).all() and np.isin(links >> 8, (0, 1)).all()


def test_stack_overflows_are_counted_not_lost():
    """the overflow scene of tests/test_gpu_edges.py: the camera walks need more than 64 stack entries; ch_chain returns their number"""
    from tests.common import Config
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), synth.procedural_sky(64, 32), 32, 24, depth=2)
    tr = TracedScene(deep.scene)
    try:
        guides_host.set_camera(tr, deep.camera)
        _, _, over = ch.chain(tr, 0, 32, 24, ch.params(8), 7, MISS_DEPTH, overflow_ok=True)
        assert over > 0
    finally:
        tr.close()


def test_the_host_build_compiles_the_products_header():
    """the dependency list recorded next to the library names the unit and the headers the product's kernel is made of"""
    from tests import host_harness as hh
    deps = hh.deps(ch.build())
    for f in ("tests/cpp/chain_host.cpp", "tests/cpp/th_scene.h", "vk_raytrace_amd/csrc/pt_chain.h", "vk_raytrace_amd/csrc/pt_guides.h", "vk_raytrace_amd/csrc/pt_query.h",
              "vk_raytrace_amd/csrc/pt_shade.h", "include/pt_types.h"):
        assert f in deps, f


# ---- 7. mutations -----------------------------------------------------------------------------------------------------------------------------------------------------
def with_library(L, test, *args):
    """run `test` with the host build replaced by the bound library L"""
    old = ch._host._lib
    ch._host._lib = L
    room_chain.cache_clear()
    try:
        test(*args)
    finally:
        ch._host._lib = old
        room_chain.cache_clear()


BREAKS = {
    "seed_not_carried": (("    seedBefore = seed;\n    hit        = chain_walk<TWO>(S, org, dir, seed, stack, counters);", "    seedBefore = seed = g.seedCamera;\n    hit        = chain_walk<TWO>(S, org, dir, seed, stack, counters);"),
                         lambda: test_every_walk_is_the_query_host_builds_closest_hit("fuzz1")),
    "dist_not_summed": (("    dist = dist + hit.x;", "    dist = hit.x;"), lambda: test_the_step_between_walks_restated_in_float32(0)),
    "tint_not_multiplied": (("    tint = tint * sf.albedo;", "    tint = sf.albedo;"), lambda: test_the_step_between_walks_restated_in_float32(0)),
    "offset_wrong_side": (("dot3(L, sf.ffnormal) > 0 ? sf.ffnormal : -sf.ffnormal", "dot3(L, sf.ffnormal) > 0 ? -sf.ffnormal : sf.ffnormal"),
                          lambda: test_the_step_between_walks_restated_in_float32(0)),
    "limit_off_by_one": (("if(cls != CHAIN_END && links == k.maxLinks)", "if(cls != CHAIN_END && links > k.maxLinks)"), lambda: test_the_step_between_walks_restated_in_float32(0)),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_a_planted_break_fails_its_test(name):
    (old, new), check = BREAKS[name]
    text = open(os.path.join(CSRC, "pt_chain.h")).read()
    assert text.count(old) == 1, name
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "pt_chain.h"), "w").write(text.replace(old, new))
        L = ch.bind(ch.compile_to(os.path.join(tmp, "libbroken.so"), header_dir=tmp))
        with pytest.raises((AssertionError, subprocess.CalledProcessError)):
            with_library(L, check)

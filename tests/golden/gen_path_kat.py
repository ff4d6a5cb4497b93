"""Mints tests/golden/path_kat.npz: the path loop held to an INDEPENDENT float64 model, pixel by pixel.

Every layer under the integrator has a numpy model of its own (gen_float_kat.py, gen_tex_kat.py, gen_surface_kat.py, gen_trace_kat.py).  This file is the glue
between them: a numpy path tracer for tiny scenes, vectorised over the pixels of an image, written from the shader text
    pathtrace.comp:97-133              seed, sample loop, sum / maxSamples, running mean          (pathtrace.rgen:72: the RTX flavour's seed)
    pathtrace.glsl:97-188              DirectLight: pSelect, light pick, punctual lights, EnvSample, the MIS weight
    pathtrace.glsl:193-343             PathTrace: miss, debug exits, unlit, absorption, emission, NEE, BSDF sample, roulette, OffsetRay, shadow ray
    pathtrace.glsl:348-387             samplePixel: jitter, camera ray, depth of field, firefly clamp
    env_sampling.glsl:126-134          EnvSample's three draws and the hdrMultiplier; :111-125 its sun branch
    common.glsl:98-113                 OffsetRay (gen_kat.offset_ray: an integer rule on the float32 bits, applied to the float32 rounding of the position)
    random.glsl:34-53, 59-65, 98-102   tea, initRandom, pcg, rand (gen_kat)
It imports numpy, the standard library and the other generators of this directory only; nothing of oracle/, tests/orc.py, tests/ref.py or vk_raytrace_amd/.
Every function takes the scalar type: np.float64 is the expectation, np.float32 only judges conditioning.

Closest hit and occlusion: brute force over all triangles (Moeller-Trumbore, t > 0, u >= 0, v >= 0, u + v <= 1) with the trace contract's rules: a
triangle of a material that is not doubleSided is culled when det = e1 . (d x e2) <= 0, the nearest accepted hit wins.  The fixture has no MASK or BLEND
material, so traversal draws no random numbers, and every node matrix is the identity.  The hit becomes a shading state through gen_surface_kat.model, the
BSDFs are gen_float_kat's, the environment lookup is gen_tex_kat's footprint and blend.
The environment's alias table is an INPUT: recorded once from the compiled reference's createEnvironmentAccel (measure_path_kat.py --table ->
path_kat_env.npz, which holds the environment and the table for the tests too; path_kat.npz does not repeat them).  The camera matrices are inputs too: lookAt / perspectiveRH_ZO with the y flip (src/scene.cpp:629-640),
inverted in float64 and rounded to float32 here; every leg is given these words.
Sun & sky: the configurations sky3 and sky0 run with in_use = 1 on the SunAndSky words of sunsky().  The model restates the miss branch (pathtrace.glsl:219-227)
and EnvSample's sun branch (env_sampling.glsl:111-125, 133: CreateCoordinateSystem on the RAW sun_direction, two draws in one quadrant, pdf = 0.5, the
hdrMultiplier, the MIS weight against that constant pdf) and calls gen_sky_kat.sun_and_sky for the colour; every branch of that function is a decision of
the pixel, and a pixel is kept only where gen_sky_kat's conditioning rules hold for every sky colour that feeds it (sky_eval).  Their 24 images are written
to path_kat_sky.npz with the words; the 39 images without sun & sky stay in path_kat.npz.

Shader quirks the model follows as written (the pixels stay kept: the behaviour is deterministic): a directional light's lightDist is length(-direction) = 1,
so its shadow ray ends one unit away (pathtrace.glsl:127-136); absorption is set again by the refraction that LEAVES the slab and only zeroed at the next
front-face hit (:265-268, :284-287); a `pdf <= 0` break in a debug mode returns the radiance (:289-296, :342).  A NaN (normalize of refract's zero vector)
ends in a non-finite pixel, which is never kept.

Kept mask, decided by the model alone.  A pixel of an image is kept when, in every frame and sample that feeds it,
  * the float32 and the float64 evaluation take every decision alike: triangle or miss, shadow verdict, light pick, rand <= pSelect, lobe, pdf > 0, roulette, clamp;
  * every rand-against-threshold comparison has the margin gen_float_kat.SPREAD (the light pick: rand * nbLights is that far from an integer; the clamp: the
    luminance is that far, relatively, from the threshold);
  * every traced ray is decided with margins: no triangle that faces the ray has it within EDGE = 1e-4 (barycentric) of one of its edges, the nearest hit is
    SEP = 1e-4 max(1, t) nearer than the runner-up, no accepted candidate lies within SEP max(1, tmax) of a shadow ray's end or within TZERO = 2e-6 of its origin;
  * the float32 result is finite and within SPREAD max(1, |float64 result|) of the float64 one.
Caps asserted here and again by the test: at most 10 % of the pixels of any image dropped, at least 50 kept pixels per branch class of TAGS.

BREAK: the rules tests/test_path_model.py's docstring lists as broken one at a time to prove that the check can fail (main(path, brk)).

Run:  python tests/golden/gen_path_kat.py   (rewrites path_kat.npz and path_kat_sky.npz; deterministic, byte-identical on every run)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_float_kat as fk  # noqa: E402
import gen_sky_kat as sk  # noqa: E402
import gen_surface_kat as gs  # noqa: E402
import gen_tex_kat as tk  # noqa: E402
from gen_kat import offset_ray, tea  # noqa: E402

SPREAD = fk.SPREAD
EDGE, SEP, TZERO = 1e-4, 1e-4, 2e-6
SKY_SPREAD = sk.SPREADS["glow"]   # a sky colour inside a path: the widest spread gen_sky_kat needs for a class the sun samples land in (glow, rise)
W, H = 46, 30            # not a multiple of the 8 x 8 block or the 32-pixel tile
FRAMES = 3
INF = 1e32               # globals.glsl:29
E_RADIANCE, E_WEIGHT, E_RAYDIR = 9, 10, 11   # host_device.h:88-102
DIRECTIONAL, POINT, SPOT = 0, 1, 2           # host_device.h:211-213
DEBUG_MODES = (("radiance", E_RADIANCE), ("weight", E_WEIGHT), ("raydir", E_RAYDIR))
BREAK = ("mis_dropped", "mis_swapped", "pselect_ignored", "env_pdf_one", "nee_no_throughput", "absorb_sign", "absorb_before_emission", "rr_no_eta2", "rr_001", "rr_095",
         "rr_no_divide", "rr_draw_missing", "clamp_weights", "lerp_1_over_frame", "jitter_frame0", "tea_swapped", "seed_unscaled", "offset_no_flip",
         "sun_pdf_one", "sun_no_hdr", "sun_three_draws", "sun_normalised", "sky_miss_no_throughput")
TAGS = ("point light", "spot light", "directional light", "nbLights 1", "nbLights 3", "pSelect 0.5, light chosen", "pSelect 1", "environment NEE with MIS",
        "light behind the surface: no shadow ray", "shadow ray occluded", "shadow ray clear", "bounded lightDist", "absorption set on entry",
        "absorption applied inside", "absorption zeroed", "thin-walled sheet", "emissive at depth 0", "emissive at depth > 0", "unlit", "metal", "pbrMode 0",
        "pbrMode 1", "miss at depth 0", "miss later", "pdf <= 0 break", "roulette death after a shadow ray", "roulette death without a shadow ray",
        "maxDepth reached", "maxDepth 0", "frame 0", "frame > 0", "aperture 0", "aperture > 0", "maxSamples 1", "maxSamples 2, ray query", "maxSamples 2, RTX",
        "clamp engaged", "clamp not engaged",
        "sky at a miss at depth 0", "sky at a later miss", "miss below the horizon (ground blend)", "sun NEE with a clear shadow ray", "sun NEE occluded",
        "sun NEE behind the surface", "sun NEE inside the disc", "sun NEE in the glow", "sun NEE outside the radius", "nbLights 0")
TAG = {name: np.uint64(1) << np.uint64(k) for k, name in enumerate(TAGS)}

LIGHT_DTYPE = np.dtype([("direction", "<f4", 3), ("range", "<f4"), ("color", "<f4", 3), ("intensity", "<f4"), ("position", "<f4", 3), ("innerConeCos", "<f4"),
                        ("outerConeCos", "<f4"), ("type", "<i4"), ("padding", "<f4", 2)])   # host_device.h:215-230
assert LIGHT_DTYPE.itemsize == 64

# name: nbLights hdrMultiplier pbrMode maxDepth aperture maxSamples variant (0 ray query, 1 RTX) firefly threshold, depths of the debug images
CONFIGS = {
    "disney3": dict(nb=3, hdr=1.0, pbr=0, depth=4, aperture=0.0, ms=1, variant=0, firefly=2.0, debug=(1, 2, 3)),
    "gltf1": dict(nb=1, hdr=0.0, pbr=1, depth=3, aperture=0.06, ms=2, variant=0, firefly=1.0e9, debug=(1, 2, 3)),
    "rtx3": dict(nb=3, hdr=0.75, pbr=1, depth=3, aperture=0.0, ms=2, variant=1, firefly=3.0, debug=(1, 2, 3)),
    "depth0": dict(nb=3, hdr=1.0, pbr=0, depth=0, aperture=0.0, ms=1, variant=0, firefly=2.0, debug=()),   # (a debug frame sets maxDepth itself: it would be disney3's)
    # Sun & sky in use (sunsky() below) instead of the environment map.  Their images go to path_kat_sky.npz: one file would pass the size limit
    "sky3": dict(nb=3, hdr=0.8, pbr=0, depth=3, aperture=0.0, ms=1, variant=0, firefly=4.0, debug=(1, 2, 3), sky=True),
    "sky0": dict(nb=0, hdr=1.0, pbr=1, depth=3, aperture=0.0, ms=1, variant=0, firefly=1.0e9, debug=(1, 2, 3), sky=True),   # no lights: no pSelect draw, every bounce samples the sun
}
SKY_CONFIGS = tuple(k for k, c in CONFIGS.items() if c.get("sky"))


def sunsky():
    """the fixture's SunAndSky words (host_device.h:258-281).  sun_direction is NOT a unit vector (EnvSample builds its frame on the raw one, sun_and_sky
    normalises it) and its rays enter through the ceiling's opening, so both shadow verdicts occur; physically_scaled_sun 0: the physically scaled disc sits
    at 1.2e-4 in float32 by itself (gen_sky_kat.SPREADS); sun_disk_scale 16 makes the sun 0.74 rad wide: the smoothstep's rise, 1.6 % of the sun draws,
    is then well-conditioned often enough for its tag, and x * x + y * y of :120 can pass 1 (z = 0); horizon_height 4 puts the horizon at 0.4 above the level, so that rays leaving through the opening
    end on both sides of it"""
    return sk.words_of(dict(sun_direction=(0.45, 0.9, 0.25), physically_scaled_sun=0, horizon_height=4.0, horizon_blur=1.5, haze=1.0, sun_disk_scale=16.0))


# ---- the fixture scene: 32 triangles ---------------------------------------------------------------------------------------------------------------------
def materials():
    out = []

    def add(name, **kw):
        m = gs.default_material()
        m["pbrMetallicFactor"] = 0.0
        for k, v in kw.items():
            m[k] = v
        out.append((name, m))

    add("white wall", pbrBaseColorFactor=(0.75, 0.75, 0.75, 1.0))
    add("red wall", pbrBaseColorFactor=(0.7, 0.2, 0.15, 1.0))
    add("green wall", pbrBaseColorFactor=(0.2, 0.65, 0.25, 1.0), pbrRoughnessFactor=0.6)
    add("emissive panel", pbrBaseColorFactor=(0.5, 0.5, 0.5, 1.0), emissiveFactor=(6.0, 5.0, 4.0), doubleSided=1)
    add("unlit", pbrBaseColorFactor=(0.2, 0.6, 0.9, 1.0), unlit=1, doubleSided=1)
    add("metal", pbrBaseColorFactor=(0.9, 0.7, 0.3, 1.0), pbrMetallicFactor=1.0, pbrRoughnessFactor=0.35, doubleSided=1)
    add("glass slab", pbrBaseColorFactor=(0.95, 0.95, 0.95, 1.0), pbrRoughnessFactor=0.25, transmissionFactor=1.0, ior=1.5, attenuationColor=(0.4, 0.8, 0.6),
        attenuationDistance=0.5, thicknessFactor=0.3, doubleSided=1, emissiveFactor=(0.3, 0.1, 0.2))   # glows: an emission add at a hit from INSIDE, absorption pending
    add("thin sheet", pbrBaseColorFactor=(0.9, 0.9, 0.6, 1.0), pbrRoughnessFactor=0.3, transmissionFactor=0.8, doubleSided=1)   # thicknessFactor 0: thin-walled
    return out


M_WHITE, M_RED, M_GREEN, M_EMIT, M_UNLIT, M_METAL, M_GLASS, M_THIN = range(8)


def quads():
    """(corner, edge 1, edge 2, material): the geometric normal is e1 x e2, a ray against it sees the front face"""
    q = [((-2, -1.5, 2), (4, 0, 0), (0, 0, -4.5), M_WHITE),          # floor
         ((-2, -1.5, -2.5), (4, 0, 0), (0, 3, 0), M_WHITE),          # back wall
         ((-2, -1.5, 2), (0, 0, -4.5), (0, 3, 0), M_RED),            # left wall
         ((2, -1.5, -2.5), (0, 0, 4.5), (0, 3, 0), M_GREEN),         # right wall
         ((2, -1.5, 2), (-4, 0, 0), (0, 3, 0), M_WHITE),             # the wall behind the camera
         ((-2, 1.5, -2.5), (2.5, 0, 0), (0, 0, 4.5), M_WHITE),       # ceiling; x in [0.5, 2] is open to the environment
         ((-1.6, 0.4, -2.45), (0.9, 0, 0), (0, 0.7, 0), M_EMIT),
         ((0.9, -1.2, -2.45), (0.8, 0, 0), (0, 0.7, 0), M_UNLIT),
         ((-1.7, -1.5, -1.2), (0.9, 0, -0.7), (0, 1.6, 0), M_METAL),
         ((1.0, -1.3, -0.2), (0.7, 0, 0.5), (0, 1.5, 0), M_THIN)]
    return [(np.array(a, np.float64), np.array(b, np.float64), np.array(c, np.float64), m) for a, b, c, m in q]


def slab():
    """the glass slab: a box of six quads wound so that every geometric normal points outwards"""
    lo, hi = np.array([-0.5, -1.3, -0.9]), np.array([0.6, 0.3, -0.5])
    d = hi - lo
    ex, ey, ez = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    return [(hi - ex - ey, ex, ey, M_GLASS), (lo + ex, -ex, ey, M_GLASS), (lo + ex, ey, ez, M_GLASS), (lo, ez, ey, M_GLASS), (lo + ey, ez, ex, M_GLASS), (lo, ex, ez, M_GLASS)]


def lights():
    out = np.zeros(3, LIGHT_DTYPE)
    out["color"], out["intensity"], out["innerConeCos"], out["outerConeCos"] = (1, 1, 1), 1.0, 1.0, np.cos(np.pi / 4)
    out[0]["type"], out[0]["position"], out[0]["intensity"], out[0]["color"], out[0]["range"] = POINT, (-0.8, 1.0, 0.5), 6.0, (1.0, 0.9, 0.8), 12.0
    sd = np.array([-1.2, -2.7, -1.6])
    out[1]["type"], out[1]["position"], out[1]["direction"], out[1]["intensity"] = SPOT, (1.2, 1.2, 0.8), sd / np.linalg.norm(sd), 1.5
    out[1]["innerConeCos"], out[1]["outerConeCos"], out[1]["color"] = 0.95, 0.8, (0.8, 0.9, 1.0)
    dd = np.array([-0.35, -1.0, -0.1])
    out[2]["type"], out[2]["direction"], out[2]["intensity"] = DIRECTIONAL, dd / np.linalg.norm(dd), 2.0
    return out


def environment():
    """4 x 2 RGBA32F texels (the size of gen_float_kat.env_sample's table), row 0 towards +y, one texel bright enough to engage the clamp"""
    e = np.ones((2, 4, 4), np.float32)
    e[0, :, :3] = [(1.0, 1.2, 1.6), (0.8, 1.0, 1.4), (14.0, 12.0, 9.0), (0.9, 1.1, 1.5)]
    e[1, :, :3] = [(0.25, 0.2, 0.15), (0.3, 0.25, 0.2), (0.2, 0.2, 0.25), (0.35, 0.3, 0.2)]
    return e


def build_scene():
    pos, nrm, idx, recs, mats_of = [], [], [], [], []

    def emit(qs):
        first_v, first_i = sum(len(p) for p in pos), sum(len(i) for i in idx)
        nv = 0
        for p0, e1, e2, _ in qs:
            n = np.cross(e1, e2)
            pos.append(np.stack([p0, p0 + e1, p0 + e1 + e2, p0 + e2]))
            nrm.append(np.tile(n / np.linalg.norm(n), (4, 1)))
            idx.append(np.array([0, 1, 2, 0, 2, 3]) + nv)
            nv += 4
        recs.append((first_v, nv, first_i, 6 * len(qs), qs[0][3]))

    for q in quads():
        emit([q])
    emit(slab())
    pos, nrm, idx = np.concatenate(pos).astype(np.float32), np.concatenate(nrm), np.concatenate(idx).astype(np.uint32)
    nv = len(pos)
    tan = np.where(np.abs(nrm[:, [1]]) > 0.9, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    tan = np.cross(nrm, np.cross(tan, nrm))
    uv = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), (nv // 4, 1))
    uv[:, 1] = ((uv[:, 1].view(np.uint32) & np.uint32(0xFFFFFFFE)) | np.uint32(1)).view(np.float32)   # handedness bit: +1
    scene = dict(position=pos, normal_code=gs.encode_oct(nrm), tangent_code=gs.encode_oct(tan), texcoord=uv, color_code=np.full(nv, 0xFFFFFFFF, np.uint32),
                 indices=idx, records=np.array(recs, np.int32), node_record=np.arange(len(recs), dtype=np.int32))
    eye = gs.affine(np.eye(3))
    scene["node_matrix"] = np.array([eye] * len(recs), np.float32)
    scene["node_inverse"] = np.array([gs.inverse_rows(eye)] * len(recs), np.float32)
    mats = materials()
    scene["materials"] = np.array([m for _, m in mats], gs.MAT_DTYPE)
    scene["material_names"] = np.array([nm for nm, _ in mats])
    scene["tex_sampler"] = np.zeros((0, 3), np.int32)
    assert len(idx) // 3 <= 32
    return scene


def camera(aspect):
    """src/scene.cpp:629-640 in float64: viewInverse, projInverse (column-major words), focalDist"""
    eye, center, up = np.array([0.1, 0.1, 1.7]), np.array([-0.1, -0.25, -2.0]), np.array([0.0, 1.0, 0.0])
    f = (center - eye) / np.linalg.norm(center - eye)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)   # glm::lookAtRH, as a mathematical (row, column) matrix
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -s @ eye, -u @ eye, f @ eye
    th, zn, zf = np.tan(np.radians(70.0) / 2), 0.001, 100000.0
    proj = np.zeros((4, 4))   # glm::perspectiveRH_ZO, [1][1] negated
    proj[0, 0], proj[1, 1], proj[2, 2], proj[3, 2], proj[2, 3] = 1 / (aspect * th), -1 / th, zf / (zn - zf), -1.0, -(zf * zn) / (zf - zn)
    vi, pi = np.linalg.inv(view), np.linalg.inv(proj)
    return vi.T.reshape(16).astype(np.float32), pi.T.reshape(16).astype(np.float32), np.float32(np.linalg.norm(center - eye))


# ---- tracing ---------------------------------------------------------------------------------------------------------------------------------------------
class Geometry:
    def __init__(self, scene, ft):
        rec = scene["records"]
        tri, inst, prim = [], [], []
        for r, (vo, _, fi, ni, _) in enumerate(rec):
            t = scene["indices"][fi:fi + ni].reshape(-1, 3).astype(np.int64) + vo
            tri.append(t); inst += [r] * len(t); prim += list(range(len(t)))
        tri = np.concatenate(tri)
        P = scene["position"].astype(ft)[tri]
        self.p0, self.e1, self.e2 = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        self.inst, self.prim = np.array(inst), np.array(prim)
        mat = np.maximum(rec[self.inst, 4], 0)
        self.cull = scene["materials"]["doubleSided"][mat] != 1   # accelstruct.cpp:148-149
        self.mat = mat


def vcross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def intersect(g, o, d, tmax=None):
    """-> (index of the nearest accepted triangle or -1, t, u, v, safe).  tmax: a shadow ray's end (per ray)"""
    with np.errstate(all="ignore"):
        D, O = d[:, None, :], o[:, None, :]
        pv = vcross(D, g.e2[None])
        det = (g.e1[None] * pv).sum(-1)
        tv = O - g.p0[None]
        u = (tv * pv).sum(-1) / det
        qv = vcross(tv, g.e1[None])
        v = (D * qv).sum(-1) / det
        t = (g.e2[None] * qv).sum(-1) / det
        m = np.minimum(np.minimum(u, v), (1 - u) - v)
        facing = ~g.cull[None] | (det > 0)
        ok = facing & (m >= 0) & (t > 0)
        lim = np.full(len(o), np.inf) if tmax is None else tmax.astype(np.float64)
        ok &= t < lim[:, None]
        tt = np.where(ok, t, np.inf)
        order = np.argsort(tt, 1, kind="stable")
        best = order[:, 0]
        pick = np.arange(len(o))
        t1, t2 = tt[pick, best], tt[pick, order[:, 1]]
        hit = np.isfinite(t1)
        reach = facing & (t > -TZERO) & (t < lim[:, None] * (1 + SEP) + SEP)
        unsafe = (reach & (np.abs(m) < EDGE)).any(1)
        unsafe |= (facing & (m > -EDGE) & (np.abs(t) < TZERO)).any(1)
        unsafe |= hit & (t2 - t1 < SEP * np.maximum(1.0, t1))
        unsafe |= (facing & (m > -EDGE) & (np.abs(t - lim[:, None]) < SEP * np.maximum(1.0, lim[:, None]))).any(1)
        unsafe |= ~np.isfinite(d).all(1) | ~np.isfinite(o).all(1)
    return np.where(hit, best, -1), np.where(hit, t1, 0), u[pick, best], v[pick, best], ~unsafe


def env_lookup(env, uv, ft):
    """texture(environmentTexture, uv): LINEAR, U repeat, V clamp to edge (gen_tex_kat: F6)"""
    h, w = env.shape[:2]
    n = len(uv)
    uv = np.where(np.isfinite(uv), uv, 0)
    on = np.ones(n, bool)
    x0, x1, a = tk.axis(uv[:, 0], w, np.full(n, tk.REPEAT), on)[:3]
    y0, y1, b = tk.axis(uv[:, 1], h, np.full(n, tk.CLAMP_TO_EDGE), on)[:3]
    img = env[:, :, :3].astype(ft)
    return tk.blend(img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1], a.astype(ft), b.astype(ft))


# ---- the path loop ---------------------------------------------------------------------------------------------------------------------------------------
class Record:
    """what decides the kept mask: the decisions in program order, the margins, the safety of every traced ray (`why` counts the pixels each rule drops); and
    the branch tags"""

    def __init__(self, n):
        self.decisions, self.ok, self.tags, self.why = [], np.ones(n, bool), np.zeros(n, np.uint64), {}

    def decide(self, mask, value):
        self.decisions.append(np.where(mask, np.asarray(value).astype(np.int64), -2))

    def need(self, mask, cond, why):
        bad = mask & ~cond
        self.ok &= ~bad
        self.why[why] = self.why.get(why, 0) + int(bad.sum())

    def tag(self, mask, name):
        self.tags = np.where(mask, self.tags | TAG[name], self.tags)


def make_state(o, V, L, seed, ft):
    """gen_surface_kat's State words (from word 17 on) as gen_float_kat's St: N is the face-forward normal"""
    s = fk.St.__new__(fk.St)
    s.ft = ft
    s.albedo, s.specular, s.anisotropy, s.metallic, s.roughness = o[:, 17:20], o[:, 45], o[:, 30], o[:, 26], o[:, 27]
    s.subsurface, s.specularTint, s.sheen, s.sheenTint, s.clearcoat = o[:, 47], o[:, 46], o[:, 41], o[:, 42:45], o[:, 31]
    s.clearcoatRoughness, s.transmission, s.ior, s.ax, s.ay, s.f0 = o[:, 32], o[:, 33], o[:, 34], o[:, 28], o[:, 29], o[:, 23:26]
    s.N, s.T, s.B, s.eta, s.thin = o[:, 6:9], o[:, 9:12], o[:, 12:15], o[:, 35], o[:, 49] != 0
    s.V, s.L, s.seed = V, L, seed
    s.back = fk.dot(o[:, 6:9], o[:, 3:6]) < 0
    return s


def sky_eval(S, dirs, mask, rec, ft):
    """sun_and_sky(_sunAndSky, dir) on the lanes of `mask` (gen_sky_kat's model) -> (colour, gen_sky_kat's branch bits).  Every branch of the function is a
    decision of the pixel; the pixel is kept only where the function is well-conditioned by gen_sky_kat's two rules: the ray is not within DOT_MARGIN of the
    sun, and moving the cosines by DOT_NUDGE moves the colour by no more than SPREAD"""
    n = len(dirs)
    words = np.ascontiguousarray(np.broadcast_to(S["sunsky"], (n, 24)), np.float32)
    d = np.where(mask[:, None] & np.isfinite(dirs).all(1)[:, None], dirs, ft(0) + np.array([0.0, 1.0, 0.0], dirs.dtype))
    with np.errstate(all="ignore"):
        res, dec, _, cosv = sk.sun_and_sky(words, d, ft)
        for v in dec.list:
            rec.decide(mask, v)
        if ft is np.float64:
            moved = np.zeros(n)
            for nudge in (-sk.DOT_NUDGE, sk.DOT_NUDGE):
                m = sk.measure(sk.sun_and_sky(words, d, ft, None, nudge)[0], res)
                moved = np.maximum(moved, np.where(np.isnan(m), np.inf, m))
            rec.need(mask, moved <= SKY_SPREAD, "sky conditioning")
            rec.need(mask, ~(cosv > 1 - sk.DOT_MARGIN), "ray at the sun")
        else:
            rec.need(mask, ~(cosv > 1), "ray at the sun")
    return res, dec.bits


def sun_sample(S, c, rng, env, rec, ft, brk):
    """EnvSample's sun branch, env_sampling.glsl:111-125, 133 -> (lightDir, radiance, pdf, gen_sky_kat's branch bits)"""
    n = len(env)
    ss = S["sunsky"]
    sd = ss[sk.W_SUN:sk.W_SUN + 3][None]                                                        # :116 the RAW sun_direction: not normalised
    if brk == "sun_normalised":
        sd = fk.f32_unit(sd)
    radius = ft(np.float32(0.00465) * np.float32(10.0)) * ft(ss[sk.W_DISK_S])                   # :114
    tb = fk.coordinate_system(np.broadcast_to(sd, (n, 3)), ft)                                  # :115-116
    x = rng.rand(env) * radius                                                                  # :118-120: two draws, one quadrant of the disc's square
    y = rng.rand(env) * radius
    if brk == "sun_three_draws":
        rng.rand(env)
    z = np.sqrt(np.maximum(ft(0), ft(1) - x * x - y * y))
    with np.errstate(all="ignore"):
        light = fk.normalize(tb[:, 0:3] * x[:, None] + tb[:, 3:6] * y[:, None] + sd.astype(ft) * z[:, None])   # :122
    rad, bits = sky_eval(S, light, env, rec, ft)                                                # :123
    if brk != "sun_no_hdr":
        rad = rad * ft(c["hdr"])                                                                # :133
    return light, rad, ft(1.0 if brk == "sun_pdf_one" else 0.5), bits                           # :124


def direct_light(S, c, st, o, d, rng, alive, rec, ft, brk):
    """pathtrace.glsl:97-188 -> (radiance, lightDir, lightDist, visible, the lanes that sampled the sun)"""
    n = len(d)
    nb = c["nb"]
    ffn, pos = o[:, 6:9], o[:, 0:3]
    p_select = ft(0.5) if c["hdr"] > 0 else ft(1.0)                                             # :113
    if brk == "pselect_ignored":
        p_select = ft(1.0)
    is_light = np.zeros(n, bool)
    if nb != 0:                                                                                 # :119 (&&: no draw without lights)
        r = rng.rand(alive)
        is_light = alive & (r <= p_select)
        rec.need(alive, np.abs(r.astype(np.float64) - float(p_select)) >= SPREAD, "rand against pSelect")
        rec.decide(alive, is_light)
        rec.tag(is_light & (p_select < 1), "pSelect 0.5, light chosen")
        rec.tag(is_light & (p_select == 1), "pSelect 1")
    light_dir, light_pdf, contrib, dist = np.zeros((n, 3), ft), np.ones(n, ft), np.zeros((n, 3), ft), np.full(n, INF, ft)
    if nb != 0:
        x = rng.rand(is_light) * ft(nb)                                                         # :124
        k = np.minimum(x, ft(nb)).astype(np.int64)
        rec.need(is_light, np.abs(x.astype(np.float64) - np.rint(x.astype(np.float64))) >= SPREAD, "light pick")
        k = np.where(is_light, np.minimum(k, nb - 1), 0)
        rec.decide(is_light, k)
        L = S["lights"][k]
        typ = L["type"]
        ldir, lpos = L["direction"].astype(ft), L["position"].astype(ft)
        ptl = np.where((typ != DIRECTIONAL)[:, None], lpos - pos, -ldir)                        # :127-134
        ld = np.sqrt(fk.dot(ptl, ptl))                                                          # :136
        with np.errstate(all="ignore"):
            ra = np.where(typ != DIRECTIONAL, fk.range_attenuation(np.stack([L["range"].astype(ft), ld], 1), ft)[:, 0], ft(1))          # :139-142
            sa = np.where(typ == SPOT, fk.spot_attenuation(np.concatenate([ptl, ldir, L["outerConeCos"].astype(ft)[:, None], L["innerConeCos"].astype(ft)[:, None]], 1), ft)[:, 0], ft(1))
            inten = (ra * sa * L["intensity"].astype(ft))[:, None] * L["color"].astype(ft)      # :148
            ndir = fk.normalize(ptl)
        light_dir, contrib, dist = np.where(is_light[:, None], ndir, light_dir), np.where(is_light[:, None], inten, contrib), np.where(is_light, ld, dist)
        for t, name in ((POINT, "point light"), (SPOT, "spot light"), (DIRECTIONAL, "directional light")):
            rec.tag(is_light & (typ == t), name)
        rec.tag(is_light, "nbLights 1" if nb == 1 else "nbLights 3")
    env = alive & ~is_light                                                                     # :155-160, env_sampling.glsl:126-134
    if c.get("sky"):
        rec.tag(alive & (nb == 0), "nbLights 0")
        sdir, erad, spdf, sky_bits = sun_sample(S, c, rng, env, rec, ft, brk)
        light_dir, contrib, light_pdf = np.where(env[:, None], sdir, light_dir), np.where(env[:, None], erad, contrib), np.where(env, spdf, light_pdf)
    else:
        xi = np.stack([rng.rand(env), rng.rand(env), rng.rand(env)], 1)
        rows = np.zeros((n, 40), np.float32)
        rows[:, 0:3], rows[:, 3], rows[:, 4] = xi, S["env"].shape[1], S["env"].shape[0]
        rows[:, 8:40] = S["env_table"].reshape(-1)
        es, (_, alias, margin) = fk.env_sample(rows, ft)
        rec.need(env, margin >= SPREAD, "alias choice")
        size = S["env"].shape[0] * S["env"].shape[1]
        xs = xi[:, 0].astype(np.float64) * size
        rec.need(env, np.abs(xs - np.rint(xs)) >= SPREAD, "alias texel")
        rec.decide(env, alias)
        erad = env_lookup(S["env"], es[:, 4:6], ft) * ft(c["hdr"])
        light_dir, contrib = np.where(env[:, None], es[:, 0:3], light_dir), np.where(env[:, None], erad, contrib)
        light_pdf = np.where(env, ft(1.0) if brk == "env_pdf_one" else es[:, 3], light_pdf)
    cosl = fk.dot(light_dir, ffn)
    visible = alive & (cosl > 0)                                                                # :162 (isSubsurface is false: :245)
    rec.need(alive, np.abs(cosl.astype(np.float64)) >= SPREAD, "light side")
    rec.decide(alive, visible)
    rec.tag(alive & ~visible, "light behind the surface: no shadow ray")
    st.V, st.L = -d, light_dir
    with np.errstate(all="ignore"):
        ev, _ = (fk.disney_eval if c["pbr"] == 0 else fk.gltf_eval)(st, ft)                      # :174
        f, pdf = ev[:, 0:3], ev[:, 3]
        a, b = (pdf, light_pdf) if brk == "mis_swapped" else (light_pdf, pdf)
        mis = np.maximum(ft(0), a * a / (b * b + a * a))                                         # :176, pbr_disney.glsl:224-229
        mis = np.where(is_light, ft(1), ft(1) if brk == "mis_dropped" else mis)
        li = (mis * np.abs(cosl))[:, None] * f * contrib / light_pdf[:, None]                    # :178
    if c.get("sky"):
        bit = lambda name: (sky_bits & sk.BIT[name]) != 0  # noqa: E731
        rec.tag(alive & env & ~visible, "sun NEE behind the surface")
        rec.tag(visible & env & bit("inside the sun radius") & ~bit("smoothstep 0"), "sun NEE inside the disc")
        rec.tag(visible & env & bit("inside the sun radius") & bit("smoothstep 0"), "sun NEE in the glow")
        rec.tag(visible & env & bit("outside the sun radius"), "sun NEE outside the radius")
    else:
        rec.tag(visible & env, "environment NEE with MIS")
    return np.where(visible[:, None], li, ft(0)), light_dir, dist, visible, env & bool(c.get("sky"))


def path_trace(S, c, org, dirs, rng, rec, ft, debug, max_depth, brk):
    """pathtrace.glsl:193-343 for all pixels -> the value PathTrace returns"""
    n = len(org)
    g = S["geometry"][ft]
    radiance, thr, absorb = np.zeros((n, 3), ft), np.ones((n, 3), ft), np.zeros((n, 3), ft)
    result = np.zeros((n, 3), ft)
    alive = np.ones(n, bool)
    o_ray, d_ray = org, dirs
    rec.tag(alive, "pbrMode 0" if c["pbr"] == 0 else "pbrMode 1")
    if max_depth == 0:
        rec.tag(alive, "maxDepth 0")
    for depth in range(max_depth):
        last = depth == max_depth - 1
        tri, t, bu, bv, safe = intersect(g, o_ray, d_ray)                                                  # :201
        rec.need(alive, safe, "closest ray")
        rec.decide(alive, tri)
        miss = alive & (tri < 0)                                                                           # :204-228
        if debug:
            val = {E_RADIANCE: radiance, E_WEIGHT: thr, E_RAYDIR: (d_ray + ft(1)) * ft(0.5)}[debug] if last else np.zeros((n, 3), ft)
        elif c.get("sky"):                                                                                 # :219-220, :227
            env, sky_bits = sky_eval(S, d_ray, miss, rec, ft)
            val = radiance + env * ft(c["hdr"]) * (ft(1) if brk == "sky_miss_no_throughput" else thr)
            rec.tag(miss, "sky at a miss at depth 0" if depth == 0 else "sky at a later miss")
            rec.tag(miss & ((sky_bits & sk.BIT["below the horizon: ground blend"]) != 0), "miss below the horizon (ground blend)")
        else:
            env = env_lookup(S["env"], fk.spherical_uv(d_ray, ft), ft)
            val = radiance + env * ft(c["hdr"]) * thr
        result = np.where(miss[:, None], val, result)
        rec.tag(miss, "miss at depth 0" if depth == 0 else "miss later")
        alive = alive & ~miss
        k = np.maximum(tri, 0)
        rows = dict(inst=g.inst[k], prim=g.prim[k], bu=bu, bv=bv, dir=d_ray)
        with np.errstate(all="ignore"):
            out, _, _ = gs.model(S["scene"], rows, ft)                                                     # :234-252
        o = out[:, 17:]
        normal, ffn, mat = o[:, 3:6], o[:, 6:9], g.mat[k]
        unlit = alive & (o[:, 48] != 0)                                                                    # :259-262
        result = np.where(unlit[:, None], radiance + o[:, 17:20] * thr, result)
        rec.tag(unlit, "unlit")
        alive = alive & ~unlit
        rec.tag(alive & (mat == M_METAL), "metal")
        rec.tag(alive & (mat == M_THIN), "thin-walled sheet")
        rec.tag(alive & (mat == M_EMIT), "emissive at depth 0" if depth == 0 else "emissive at depth > 0")
        front = fk.dot(normal, ffn) > 0                                                                    # :265-268
        had = (absorb != 0).any(1)
        rec.tag(alive & front & had, "absorption zeroed")
        absorb = np.where((alive & front)[:, None], ft(0), absorb)
        sign = ft(1) if brk == "absorb_sign" else ft(-1)
        if brk == "absorb_before_emission":
            thr = np.where(alive[:, None], thr * np.exp(sign * absorb * t.astype(ft)[:, None]), thr)
        radiance = np.where(alive[:, None], radiance + o[:, 20:23] * thr, radiance)                        # :271
        if brk != "absorb_before_emission":
            thr = np.where(alive[:, None], thr * np.exp(sign * absorb * t.astype(ft)[:, None]), thr)       # :274
        rec.tag(alive & (absorb != 0).any(1), "absorption applied inside")
        st = make_state(o, -d_ray, -d_ray, rng.s, ft)
        vrad, ldir, ldist, visible, sun_nee = direct_light(S, c, st, o, d_ray, rng, alive, rec, ft, brk)       # :277
        if brk != "nee_no_throughput":
            vrad = vrad * thr                                                                              # :278
        st.seed = rng.s
        with np.errstate(all="ignore"):
            sm, (seed2, branch, margin) = (fk.disney_sample if c["pbr"] == 0 else fk.gltf_sample)(st, ft)  # :281
        rng.s = np.where(alive, seed2, rng.s)
        L, f, pdf = sm[:, 0:3], sm[:, 3:6], sm[:, 6]
        rec.need(alive, margin >= SPREAD, "lobe choice")
        rec.decide(alive, branch)
        cos_l = fk.dot(ffn, L)
        inward = alive & (cos_l < 0)                                                                       # :284-287
        with np.errstate(all="ignore"):
            absorb = np.where(inward[:, None], -np.log(o[:, 36:39]) / o[:, 39:40], absorb)
        rec.tag(inward & front & (mat == M_GLASS), "absorption set on entry")
        good = pdf > 0                                                                                     # :289-296
        rec.decide(alive, good)
        rec.need(alive, np.abs(cos_l.astype(np.float64)) >= SPREAD, "sampled side")   # decides the lobes' `back` exit (pdf = 0 exactly), the absorption and the offset
        brk_pdf = alive & ~good
        result = np.where(brk_pdf[:, None], radiance, result)
        rec.tag(brk_pdf, "pdf <= 0 break")
        alive = alive & good
        with np.errstate(all="ignore"):
            thr = np.where(alive[:, None], thr * f * np.abs(cos_l)[:, None] / pdf[:, None], thr)
        if debug and last:                                                                                 # :299-307
            val = {E_RADIANCE: vrad, E_WEIGHT: thr, E_RAYDIR: (L + ft(1)) * ft(0.5)}[debug]
            result = np.where(alive[:, None], val, result)
            rec.tag(alive, "maxDepth reached")
            alive = np.zeros(n, bool)
            break
        eta = o[:, 35]
        eta2 = ft(1) if brk == "rr_no_eta2" else eta * eta
        lo, hi = ft(0.01 if brk == "rr_001" else 0.001), ft(0.9 if brk == "rr_095" else 0.95)
        pcont = np.minimum(thr.max(1) * eta2 + lo, hi)                                                     # :311-313 (RR_DEPTH 0)
        d_ray = np.where(alive[:, None], L, d_ray)                                                         # :317-318
        flip = fk.dot(L, ffn) > 0
        if brk == "offset_no_flip":
            flip = np.ones(n, bool)
        on = np.where(flip[:, None], ffn, -ffn)
        with np.errstate(all="ignore"):
            nxt = offset_ray(o[:, 0:3].astype(np.float32), on.astype(np.float32)).astype(ft)
        o_ray = np.where(alive[:, None], nxt, o_ray)
        shadow = alive & visible                                                                           # :322-331
        s_tri, _, _, _, s_safe = intersect(g, o_ray, ldir, ldist)
        rec.need(shadow, s_safe, "shadow ray")
        lit = shadow & (s_tri < 0)
        rec.decide(shadow, lit)
        rec.tag(shadow & ~lit, "shadow ray occluded")
        rec.tag(lit, "shadow ray clear")
        rec.tag(shadow & ~lit & sun_nee, "sun NEE occluded")
        rec.tag(lit & sun_nee, "sun NEE with a clear shadow ray")
        rec.tag(shadow & (ldist < ft(1e30)), "bounded lightDist")
        radiance = np.where(lit[:, None], radiance + vrad, radiance)
        draw = alive & visible if brk == "rr_draw_missing" else alive                                      # :335-337
        r = rng.rand(draw)
        r = np.where(draw, r, ft(0))
        dead = alive & (r >= pcont)
        rec.need(alive, np.abs(r.astype(np.float64) - pcont.astype(np.float64)) >= SPREAD, "roulette")
        rec.decide(alive, dead)
        rec.tag(dead & visible, "roulette death after a shadow ray")
        rec.tag(dead & ~visible, "roulette death without a shadow ray")
        result = np.where(dead[:, None], radiance, result)
        alive = alive & ~dead
        if brk != "rr_no_divide":
            thr = np.where(alive[:, None], thr / pcont[:, None], thr)
        if last:
            rec.tag(alive, "maxDepth reached")
    return np.where(alive[:, None], radiance, result)                                                     # :342


def render_frame(S, c, cam, frame, ft, debug=0, max_depth=None, brk=None):
    """pathtrace.comp:87-133 up to pixelColor /= maxSamples -> (pixel colours (n, 3), Record)"""
    max_depth = c["depth"] if max_depth is None else max_depth
    n = W * H
    px, py = np.arange(n) % W, np.arange(n) // W
    ms = c["ms"]
    scale = 1 if (c["variant"] == 1 or brk == "seed_unscaled") else ms                          # pathtrace.comp:97 / pathtrace.rgen:72 + random.glsl:50-53
    a, b = (W * py + px).astype(np.uint64), np.full(n, frame * scale, np.uint64)
    rng = fk.Draws(tea(b, a) if brk == "tea_swapped" else tea(a, b), ft)
    rec = Record(n)
    all_ = np.ones(n, bool)
    rec.tag(all_, "frame 0" if frame == 0 else "frame > 0")
    rec.tag(all_, "aperture 0" if c["aperture"] == 0 else "aperture > 0")
    rec.tag(all_, "maxSamples 1" if ms == 1 else ("maxSamples 2, RTX" if c["variant"] == 1 else "maxSamples 2, ray query"))
    vi, pi = cam["viewInverse"].astype(ft).reshape(4, 4).T, cam["projInverse"].astype(ft).reshape(4, 4).T   # (row, column)
    total = np.zeros((n, 3), ft)
    for _ in range(ms):
        if frame == 0 and brk != "jitter_frame0":                                               # pathtrace.glsl:353
            jx, jy = np.full(n, ft(0.5)), np.full(n, ft(0.5))
        else:
            jx = rng.rand()
            jy = rng.rand()
        ux, uy = (px.astype(ft) + jx) / ft(W), (py.astype(ft) + jy) / ft(H)                     # :356-358
        dx, dy = ux * ft(2) - ft(1), uy * ft(2) - ft(1)
        origin = vi[:3, 3]                                                                      # :361-363
        tgt = np.stack([pi[r, 0] * dx + pi[r, 1] * dy + pi[r, 2] + pi[r, 3] for r in range(3)], 1)
        tgt = fk.normalize(tgt)
        direction = tgt @ vi[:3, :3].T
        focal = direction * cam["focalDist"].astype(ft)                                         # :366-372
        r1, r2 = rng.rand() * ft(2 * fk.PI), rng.rand() * ft(c["aperture"])
        lens = (np.cos(r1)[:, None] * vi[:3, 0] + np.sin(r1)[:, None] * vi[:3, 1]) * np.sqrt(r2)[:, None]
        radiance = path_trace(S, c, origin[None, :] + lens, fk.normalize(focal - lens), rng, rec, ft, debug, max_depth, brk)   # :374-377
        wts = (0.3, 0.6, 0.1) if brk == "clamp_weights" else (0.212671, 0.715160, 0.072169)
        lum = radiance[:, 0] * ft(wts[0]) + radiance[:, 1] * ft(wts[1]) + radiance[:, 2] * ft(wts[2])   # :380-384
        thr = ft(c["firefly"])
        clamp = lum > thr
        with np.errstate(all="ignore"):
            radiance = np.where(clamp[:, None], radiance * (thr / lum)[:, None], radiance)
            rec.need(all_, np.abs(lum.astype(np.float64) - float(thr)) >= SPREAD * float(thr), "clamp")
        rec.decide(all_, clamp)
        rec.tag(clamp, "clamp engaged")
        rec.tag(~clamp, "clamp not engaged")
        total = total + radiance
    return total / ft(ms), rec


def accumulate(old, new, frame, ft, brk=None):
    """pathtrace.comp:122-133: mix(old, new, 1 / (frame + 1))"""
    if frame == 0:
        return new
    a = ft(1) / ft(frame if brk == "lerp_1_over_frame" else frame + 1)
    return old * (ft(1) - a) + new * a


def both(S, c, cam, frame, **kw):
    """one frame in float64 and in float32 -> (float64 colours, float32 colours, stable mask, tags)"""
    v64, r64 = render_frame(S, c, cam, frame, np.float64, **kw)
    v32, r32 = render_frame(S, c, cam, frame, np.float32, **kw)
    same = np.ones(W * H, bool)
    assert len(r64.decisions) == len(r32.decisions)
    for a, b in zip(r64.decisions, r32.decisions):
        same &= a == b
    return v64, v32, same & r64.ok & r32.ok, r64.tags


def close(v32, v64):
    with np.errstate(all="ignore"):
        return np.isfinite(v32).all(1) & np.isfinite(v64).all(1) & (np.abs(v32.astype(np.float64) - v64) <= SPREAD * np.maximum(1.0, np.abs(v64))).all(1)


def load_env_table():
    path = os.path.join(HERE, "path_kat_env.npz")
    assert os.path.exists(path), "run tests/golden/measure_path_kat.py --table first: the alias table is recorded from the compiled reference"
    with np.load(path) as z:
        assert np.array_equal(z["env"], environment()), "path_kat_env.npz was recorded for another environment"
        return z["env_table"].view(np.float32)   # (texels, 4) words: alias q pdf aliasPdf


def mint(brk=None):
    scene = build_scene()
    table = load_env_table()
    S = dict(scene=scene, lights=lights(), env=environment(), env_table=table, sunsky=sunsky(), geometry={ft: Geometry(scene, ft) for ft in (np.float64, np.float32)})
    vi, pi, fd = camera(W / H)
    cam = dict(viewInverse=vi, projInverse=pi, focalDist=fd)
    out = dict(scene)
    out.update(lights=S["lights"], viewInverse=vi, projInverse=pi, focalDist=fd,   # (the environment and its table stay in path_kat_env.npz: one committed copy)
               size=np.array([W, H], np.int32), tag_names=np.array(TAGS), config_names=np.array(list(CONFIGS)))
    names = []
    for cn, c in CONFIGS.items():
        out["cfg_" + cn] = np.array([c["nb"], c["hdr"], c["pbr"], c["depth"], c["aperture"], c["ms"], c["variant"], c["firefly"]], np.float64)
        acc64 = acc32 = None
        stable, tags = np.ones(W * H, bool), np.zeros(W * H, np.uint64)
        for frame in range(FRAMES):
            v64, v32, ok, tg = both(S, c, cam, frame, brk=brk)
            acc64, acc32 = accumulate(acc64, v64, frame, np.float64, brk), accumulate(acc32, v32, frame, np.float32, brk)
            stable, tags = stable & ok, tags | tg
            name = f"{cn}_acc{frame + 1}"
            out["img_" + name], out["kept_" + name], out["tags_" + name] = acc64.reshape(H, W, 3), (stable & close(acc32, acc64)).reshape(H, W), tags.reshape(H, W)
            names.append(name)
        for k in c["debug"]:
            for mn, mode in DEBUG_MODES:
                v64, v32, ok, tg = both(S, c, cam, 0, debug=mode, max_depth=k, brk=brk)
                name = f"{cn}_{mn}{k}"
                out["img_" + name], out["kept_" + name], out["tags_" + name] = v64.reshape(H, W, 3), (ok & close(v32, v64)).reshape(H, W), tg.reshape(H, W)
                names.append(name)
    out["image_names"] = np.array(names)
    out["sunsky"] = S["sunsky"]
    return out


def split(out):
    """-> (what path_kat.npz holds, what path_kat_sky.npz holds: the images of SKY_CONFIGS, their cfg_ words and the SunAndSky words).  tests/path_kat_io.py
    load() puts them together again"""
    is_sky = lambda k: k.split("_", 1)[-1].split("_")[0] in SKY_CONFIGS and k.split("_", 1)[0] in ("img", "kept", "tags", "cfg")  # noqa: E731
    base = {k: v for k, v in out.items() if not is_sky(k) and k != "sunsky"}
    sky = {k: v for k, v in out.items() if is_sky(k)}
    base["image_names"] = np.array([n for n in out["image_names"] if n.split("_")[0] not in SKY_CONFIGS])
    base["config_names"] = np.array([n for n in out["config_names"] if n not in SKY_CONFIGS])
    sky["sky_image_names"] = np.array([n for n in out["image_names"] if n.split("_")[0] in SKY_CONFIGS])
    sky["sky_config_names"], sky["sunsky"] = np.array(SKY_CONFIGS), out["sunsky"]
    return base, sky


def check_caps(out, report=False):
    """the two caps of the kept mask -> (worst dropped fraction, kept pixels per tag); asserts them"""
    drops, counts = {}, np.zeros(len(TAGS), np.int64)
    for name in out["image_names"]:
        kept = out["kept_" + name]
        drops[str(name)] = 1.0 - kept.mean()
        tg = out["tags_" + name][kept]
        for k in range(len(TAGS)):
            counts[k] += int(((tg >> np.uint64(k)) & np.uint64(1)).sum())
    if report:
        print("dropped: " + ", ".join(f"{n} {d:.1%}" for n, d in drops.items()))
        print("kept pixels per branch class: " + ", ".join(f"{TAGS[k]} {counts[k]}" for k in range(len(TAGS))))
    over = [f"{n}: {d:.1%}" for n, d in drops.items() if d > 0.10]
    assert not over, "images with more than 10 % of the pixels dropped: " + "; ".join(over)
    short = [f"{TAGS[k]}: {counts[k]}" for k in range(len(TAGS)) if counts[k] < 50]
    assert not short, "branch classes with fewer than 50 kept pixels: " + "; ".join(short)
    return max(drops.values()), counts


def main(path=None, brk=None, caps=True):
    assert brk is None or brk in BREAK
    out = mint(brk)
    if caps:
        worst, counts = check_caps(out, report=True)
        print(f"worst image drops {worst:.2%}; fewest kept pixels of a branch class: {TAGS[int(counts.argmin())]} {counts.min()}")
    path = path or os.path.join(HERE, "path_kat.npz")
    for p, part in zip((path, path[:-4] + "_sky.npz"), split(out)):
        gs.write_npz(p, part)
        print("wrote", p, os.path.getsize(p), "bytes,", sum(k.startswith("img_") for k in part), "images of", W, "x", H)


if __name__ == "__main__":
    main()

"""Mints the FLOAT known answers in tests/golden/float_kat.npz: an independent float64 model of the shading math.

Every other float check of this project compares the HIP code, the CPU oracle and the reference's compiled shaders with each other, and all
three take their GLSL built-ins from code written here.  This file is the leg that shares nothing with them: numpy only, written from the
reference's shader text (file:line cited per function) and from the GLSL specification's formulas for the built-ins, importing nothing of
oracle/, tests/orc.py, tests/ref.py or vk_raytrace_amd/.  Random numbers come from gen_kat.pcg_step / word_to_float (pinned by tests/test_kat.py).

Every function takes the scalar type `ft`, so the same code runs in np.float64 (the expectation) and in np.float32 (only to judge conditioning).

Functions (tests/test_float_kat.py holds oracle, compiled reference, the product's host build and the device probe to them):
  reflect, refract, mix, smoothstep     GLSL 4.60 specification 8.3 / 8.5 (formulas restated below)
  step, clamp, sign, fract, mod, atan(y, x), roundEven   GLSL 4.60 specification 8.1 / 8.3
  DisneyEval, DisneySample              shaders/pbr_disney.glsl:68-229 (terms), :320-410 (lobes), :414-520, :524-599
  PbrEval, PbrSample                    shaders/pbr_gltf.glsl:31-199 (terms), :204-361 (lobes), :365-434, :439-554
  GetSphericalUv, CreateCoordinateSystem  shaders/common.glsl:67-74, :80-92
  getRangeAttenuation, getSpotAttenuation shaders/punctual.glsl:28-36, :39-51
  cross, normalize, mat4 * vec4, vec4 * mat4, mat4x3 * vec4, vec3 * mat4x3, mat3 * vec3   GLSL 4.60 specification 5.10 / 8.5 (column-major)
  Environment_sample                    shaders/env_sampling.glsl:38-99 on a hand-made EnvAccel table
  EnvSample's sun-disk direction        shaders/env_sampling.glsl:111-125
  linearTosRGB, sRGBToLinear, toneMapUncharted, toneMapHejlRichard, toneMapACES, toneMap   shaders/tonemapping.glsl:29-105
  rand                                  shaders/random.glsl:59-65, 98-102 (through gen_kat)
sun_and_sky (shaders/sun_and_sky.glsl) has a generator of its own, gen_sky_kat.py, which takes its sphere directions from sky_dirs() here; EnvSample's sun branch
as the path loop runs it is in gen_path_kat.py (configurations sky3, sky0).
The shading state is the 22-float material vector + frame of the function-level probes (oracle/pt_oracle.cpp orc_fill_state): ffnormal = normal.

Conditioning filter, decided by the model alone (never by the code under test): a state is KEPT when the model's float32 evaluation is within
SPREAD of its float64 evaluation in the error measure |a - b| / (|b| + 1e-6) (absolute error for the sampled unit vector L), takes the same branch,
and -- for the sample functions -- every `rand() < threshold` comparison it evaluates has a margin of at least SPREAD.  States with dot(N, V) <= 0
are outside the model's domain (the renderer's face-forward normal excludes them): stored for the bit-identity checks, never kept, not counted.
Caps asserted here and again by the test: at most 2 % of the in-domain states of a function dropped, at least 50 kept states per sample branch,
every edge state kept or named with the reason.

Where the shader itself is questionable the model follows it as written: normalize() of refract()'s zero vector (k < 0) gives NaN in DisneySample's
transmission branch; such states have a non-finite expectation and are dropped (they count against the cap).

Run:  python tests/golden/gen_float_kat.py   (rewrites float_kat.npz; deterministic)
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_kat import pcg_step, word_to_float  # noqa: E402

SPREAD = 1e-5
N_BSDF = 1300
PI = 3.14159265358979323846


# ---- random inputs: the pinned PCG stream --------------------------------------------------------------------------------------------------
class Stream:
    """n parallel PCG streams (shaders/random.glsl:59-65, 98-102)"""

    def __init__(self, n, salt):
        self.s = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)).astype(np.uint32)
        for _ in range(3):
            self.s, _ = pcg_step(self.s)

    def u(self, lo=0.0, hi=1.0):
        self.s, w = pcg_step(self.s)
        return lo + (hi - lo) * word_to_float(w).astype(np.float64)

    def word(self):
        self.s, w = pcg_step(self.s)
        return w

    def unit(self):
        z, phi = 1.0 - 2.0 * self.u(), 2.0 * PI * self.u()
        r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def f32_unit(v):
    v = v.astype(np.float32)
    return (v / np.sqrt((v * v).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)


# ---- GLSL built-ins by the specification's formulas -------------------------------------------------------------------------------------------
def dot(a, b):
    return (a * b).sum(-1)


def col(x):
    return x[..., None]


def normalize(v):
    return v / col(np.sqrt(dot(v, v)))


def cross(a, b):  # GLSL 8.5: (x[1]y[2] - y[1]x[2], x[2]y[0] - y[2]x[0], x[0]y[1] - y[0]x[1])
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1)


def reflect(I, N):  # GLSL 8.5: I - 2 dot(N, I) N
    return I - col(I.dtype.type(2) * dot(N, I)) * N


def refract(I, N, eta):  # GLSL 8.5: k = 1 - eta^2 (1 - dot(N, I)^2); k < 0 ? 0 : eta I - (eta dot(N, I) + sqrt(k)) N
    ft = I.dtype.type
    d = dot(N, I)
    k = ft(1) - eta * eta * (ft(1) - d * d)
    with np.errstate(invalid="ignore"):
        r = col(eta) * I - col(eta * d + np.sqrt(k)) * N
    return np.where(col(k < 0), ft(0), r)


def mix(a, b, t):  # GLSL 8.3: x (1 - a) + y a
    return a * (a.dtype.type(1) - t) + b * t


def clamp(x, lo, hi):  # GLSL 8.3: min(max(x, lo), hi)
    return np.minimum(np.maximum(x, x.dtype.type(lo)), x.dtype.type(hi))


def smoothstep(e0, e1, x):  # GLSL 8.3: t = clamp((x - e0) / (e1 - e0), 0, 1); t t (3 - 2 t)
    t = clamp((x - e0) / (e1 - e0), 0, 1)
    return t * t * (x.dtype.type(3) - x.dtype.type(2) * t)


# ---- shaders/common.glsl ----------------------------------------------------------------------------------------------------------------------
def spherical_uv(v, ft):  # common.glsl:67-74
    v = v.astype(ft)
    with np.errstate(invalid="ignore"):
        gamma = np.arcsin(-v[:, 1])
    theta = np.arctan2(v[:, 2], v[:, 0])
    return np.stack([theta * ft(1 / PI) * ft(0.5) + ft(0.5), gamma * ft(1 / PI) + ft(0.5)], 1)


def coordinate_system(N, ft):  # common.glsl:80-92
    N = N.astype(ft)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    a = np.stack([-x * y, ft(1) - y * y, -y * z], 1)
    b = np.stack([-x * z, -y * z, ft(1) - z * z], 1)
    T = normalize(np.where(col(np.abs(z) > ft(np.float32(0.99999))), a, b))
    return np.concatenate([T, cross(T, N)], 1)


# ---- shaders/punctual.glsl ----------------------------------------------------------------------------------------------------------------------
def range_attenuation(rd, ft):  # punctual.glsl:28-36
    r, d = rd[:, 0].astype(ft), rd[:, 1].astype(ft)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.maximum(np.minimum(ft(1) - (d / r) ** ft(4), ft(1)), ft(0)) / d ** ft(2)
    return col(np.where(r <= 0, ft(1), a))


def spot_attenuation(x, ft):  # punctual.glsl:39-51
    x = x.astype(ft)
    c = dot(normalize(x[:, 3:6]), normalize(-x[:, 0:3]))
    outer, inner = x[:, 6], x[:, 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = smoothstep(outer, inner, c)
    return col(np.where(c > outer, np.where(c < inner, s, ft(1)), ft(0)))


# ---- shaders/pbr_disney.glsl: terms ----------------------------------------------------------------------------------------------------------
class St:
    """the shading state of a row block: material vector + frame, in scalar type ft"""

    def __init__(self, rows, ft):
        r = rows.astype(ft)
        self.ft = ft
        self.albedo, self.specular, self.anisotropy, self.metallic, self.roughness = r[:, 0:3], r[:, 3], r[:, 4], r[:, 5], r[:, 6]
        self.subsurface, self.specularTint, self.sheen, self.sheenTint, self.clearcoat = r[:, 7], r[:, 8], r[:, 9], r[:, 10:13], r[:, 13]
        self.clearcoatRoughness, self.transmission, self.ior, self.ax, self.ay, self.f0 = r[:, 14], r[:, 15], r[:, 16], r[:, 17], r[:, 18], r[:, 19:22]
        self.N, self.T, self.B, self.eta, self.thin = r[:, 22:25], r[:, 25:28], r[:, 28:31], r[:, 31], rows[:, 32] != 0
        self.V, self.L = r[:, 33:36], r[:, 36:39]
        self.seed = rows[:, 39].copy().view(np.uint32)
        self.back = np.zeros(len(rows), bool)   # dot(ffnormal, normal) < 0; never in this state (ffnormal == normal).  gen_path_kat.py builds states where it happens.


def state_of(rows, ft):
    """the probe rows as a state; a state built elsewhere (gen_path_kat.py: from a hit, in ft throughout) passes through"""
    return rows if isinstance(rows, St) else St(rows, ft)


def schlick_fresnel(u):  # :114-119
    m = clamp(u.dtype.type(1) - u, 0, 1)
    m2 = m * m
    return m2 * m2 * m


def dielectric_fresnel(ci, eta):  # :123-137
    ft = ci.dtype.type
    s2 = eta * eta * (ft(1) - ci * ci)
    ct = np.sqrt(np.maximum(ft(1) - s2, ft(0)))
    rs = (eta * ct - ci) / (eta * ct + ci)
    rp = (eta * ci - ct) / (eta * ci + ct)
    return np.where(s2 > 1, ft(1), ft(0.5) * (rs * rs + rp * rp))


def gtr1(ndh, a):  # :141-148
    ft = ndh.dtype.type
    a2 = a * a
    t = ft(1) + (a2 - ft(1)) * ndh * ndh
    return np.where(a >= 1, ft(1 / PI), (a2 - ft(1)) / (ft(PI) * np.log(a2) * t))


def gtr2(ndh, a):  # :152-157
    ft = ndh.dtype.type
    a2 = a * a
    t = ft(1) + (a2 - ft(1)) * ndh * ndh
    return a2 / (ft(PI) * t * t)


def gtr2_aniso(ndh, hdx, hdy, ax, ay):  # :161-167
    a, b = hdx / ax, hdy / ay
    c = a * a + b * b + ndh * ndh
    return ndh.dtype.type(1) / (ndh.dtype.type(PI) * ax * ay * c * c)


def smith_ggx(ndv, alpha):  # :171-176
    a, b = alpha * alpha, ndv * ndv
    return ndv.dtype.type(1) / (ndv + np.sqrt(a + b - a * b))


def smith_ggx_aniso(ndv, vdx, vdy, ax, ay):  # :180-186
    a, b = vdx * ax, vdy * ay
    return ndv.dtype.type(1) / (ndv + np.sqrt(a * a + b * b + ndv * ndv))


def cosine_hemisphere(r1, r2):  # :190-200
    ft = r1.dtype.type
    r, phi = np.sqrt(r1), ft(2 * PI) * r2
    x, y = r * np.cos(phi), r * np.sin(phi)
    return np.stack([x, y, np.sqrt(np.maximum(ft(0), ft(1) - x * x - y * y))], 1)


def uniform_hemisphere(r1, r2):  # :204-210
    ft = r1.dtype.type
    r, phi = np.sqrt(np.maximum(ft(0), ft(1) - r1 * r1)), ft(2 * PI) * r2
    return np.stack([r * np.cos(phi), r * np.sin(phi), r1], 1)


def sample_gtr1(rgh, r1, r2):  # :68-81 (r2 is not used there either)
    ft = r1.dtype.type
    a = np.maximum(ft(0.001), rgh)
    a2 = a * a
    phi = r1 * ft(2 * PI)
    ct = np.sqrt((ft(1) - a2 ** (ft(1) - r1)) / (ft(1) - a2))
    st = clamp(np.sqrt(ft(1) - ct * ct), 0, 1)
    return np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1)


def sample_gtr2_aniso(ax, ay, r1, r2):  # :85-94
    ft = r1.dtype.type
    phi = r1 * ft(2 * PI)
    tan = np.sqrt(r2 / (ft(1) - r2))
    return np.stack([tan * (ax * np.cos(phi)), tan * (ay * np.sin(phi)), np.ones_like(r1)], 1)


def sample_gtr2(rgh, r1, r2, floor=True):  # :98-110; pbr_gltf.glsl:189-199 GgxSampling is the same without the floor on the roughness
    ft = r1.dtype.type
    a = np.maximum(ft(0.001), rgh) if floor else rgh
    phi = r1 * ft(2 * PI)
    ct = np.sqrt((ft(1) - r2) / (ft(1) + (a * a - ft(1)) * r2))
    st = clamp(np.sqrt(ft(1) - ct * ct), 0, 1)
    return np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1)


def to_world(s, h, nsign=1):
    return s.T * col(h[:, 0]) + s.B * col(h[:, 1]) + s.N * col(h[:, 2] * s.ft(nsign))


# ---- shaders/pbr_disney.glsl: lobes.  Each returns (f, pdf); `pdf0` is the value the inout pdf keeps on the early return ------------------------
def d_reflection(s, eta, V, N, L, H, pdf0):  # :320-332
    F = dielectric_fresnel(dot(V, H), eta)
    D = gtr2(dot(N, H), s.roughness)
    pdf = D * dot(N, H) * F / (s.ft(4) * dot(V, H))
    G = smith_ggx(np.abs(dot(N, L)), s.roughness) * smith_ggx(dot(N, V), s.roughness)
    back = dot(N, L) < 0
    return np.where(col(back), s.ft(0), s.albedo * col(F * D * G)), np.where(back, pdf0, pdf)


def d_refraction(s, eta, V, N, L, H):  # :336-347
    ft = s.ft
    F = dielectric_fresnel(np.abs(dot(V, H)), eta)
    D = gtr2(dot(N, H), s.roughness)
    den = dot(L, H) * eta + dot(V, H)
    pdf = D * dot(N, H) * (ft(1) - F) * np.abs(dot(L, H)) / (den * den)
    G = smith_ggx(np.abs(dot(N, L)), s.roughness) * smith_ggx(dot(N, V), s.roughness)
    return s.albedo * col((ft(1) - F) * D * G * np.abs(dot(V, H)) * np.abs(dot(L, H)) * ft(4) * eta * eta / (den * den)), pdf


def d_specular(s, Cspec0, V, N, L, H, pdf0):  # :351-364
    ft = s.ft
    D = gtr2_aniso(dot(N, H), dot(H, s.T), dot(H, s.B), s.ax, s.ay)
    pdf = D * dot(N, H) / (ft(4) * dot(V, H))
    F = mix(Cspec0, np.ones_like(Cspec0), col(schlick_fresnel(dot(L, H))))
    G = smith_ggx_aniso(dot(N, L), dot(L, s.T), dot(L, s.B), s.ax, s.ay) * smith_ggx_aniso(dot(N, V), dot(V, s.T), dot(V, s.B), s.ax, s.ay)
    back = dot(N, L) < 0
    return np.where(col(back), ft(0), F * col(D * G)), np.where(back, pdf0, pdf)


def d_clearcoat(s, V, N, L, H, pdf0):  # :368-380
    ft = s.ft
    D = gtr1(dot(N, H), s.clearcoatRoughness)
    pdf = D * dot(N, H) / (ft(4) * dot(V, H))
    F = mix(np.full_like(D, ft(0.04)), np.ones_like(D), schlick_fresnel(dot(L, H)))
    G = smith_ggx(dot(N, L), np.full_like(D, ft(0.25))) * smith_ggx(dot(N, V), np.full_like(D, ft(0.25)))
    back = dot(N, L) < 0
    return np.where(col(back), ft(0), col(ft(0.25) * s.clearcoat * F * D * G) * np.ones((1, 3), ft)), np.where(back, pdf0, pdf)


def d_diffuse(s, Csheen, V, N, L, H, pdf0):  # :384-398
    ft = s.ft
    pdf = dot(N, L) * ft(1 / PI)
    FL, FV, FH = schlick_fresnel(dot(N, L)), schlick_fresnel(dot(N, V)), schlick_fresnel(dot(L, H))
    Fd90 = ft(0.5) + ft(2) * dot(L, H) * dot(L, H) * s.roughness
    Fd = mix(np.ones_like(FL), Fd90, FL) * mix(np.ones_like(FL), Fd90, FV)
    f = (col(ft(1 / PI) * Fd * (ft(1) - s.subsurface)) * s.albedo + col(FH * s.sheen) * Csheen) * col(ft(1) - s.metallic)
    back = dot(N, L) < 0
    return np.where(col(back), ft(0), f), np.where(back, pdf0, pdf)


def d_subsurface(s, V, N, L):  # :402-410
    ft = s.ft
    FL, FV = schlick_fresnel(np.abs(dot(N, L))), schlick_fresnel(dot(N, V))
    Fd = (ft(1) - ft(0.5) * FL) * (ft(1) - ft(0.5) * FV)
    return np.sqrt(s.albedo) * col(s.subsurface * ft(1 / PI) * Fd * (ft(1) - s.metallic) * (ft(1) - s.transmission)), np.full_like(FL, ft(1 / (2 * PI)))


def d_spec_tint(s):  # :426-431 == :576-581
    ft = s.ft
    lum = ft(0.3) * s.albedo[:, 0] + ft(0.6) * s.albedo[:, 1] + ft(0.1) * s.albedo[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        tint = np.where(col(lum > 0), s.albedo / col(lum), ft(1))
    return mix(col(s.specular * ft(0.08)) * mix(np.ones_like(tint), tint, col(s.specularTint)), s.albedo, col(s.metallic))


def half_vector(s, V, N, L):  # :526-534 == pbr_gltf.glsl:367-375
    H = np.where(col(dot(N, L) < 0), normalize(L * col(s.ft(1) / s.eta) + V), normalize(L + V))
    return np.where(col(dot(N, H) < 0), -H, H)


def disney_eval(rows, ft):  # :524-599
    s = state_of(rows, ft)
    V, N, L = s.V, s.N, s.L
    z1, z3 = np.zeros(len(s.V), ft), np.zeros((len(s.V), 3), ft)
    H = half_vector(s, V, N, L)
    dr, psr, tw = ft(0.5) * (ft(1) - s.metallic), ft(1) / (ft(1) + s.clearcoat), (ft(1) - s.metallic) * s.transmission
    back = dot(N, L) < 0
    fr, pr = d_refraction(s, s.eta, V, N, L, H)
    fl, pl = d_reflection(s, s.eta, V, N, L, H, z1)
    bsdf = np.where(col(tw > 0), np.where(col(back), fr, fl), z3)
    bsdf_pdf = np.where(tw > 0, np.where(back, pr, pl), z1)
    fs, ps = d_subsurface(s, V, N, L)
    fd, pd = d_diffuse(s, s.sheenTint, V, N, L, H, z1)
    fp, pp = d_specular(s, d_spec_tint(s), V, N, L, H, z1)
    fc, pc = d_clearcoat(s, V, N, L, H, z1)
    front_f = (fd + fp) + fc
    front_p = (pd * (ft(1) - s.subsurface) * dr + pp * psr * (ft(1) - dr)) + pc * (ft(1) - psr) * (ft(1) - dr)
    sub = s.subsurface > 0
    brdf = np.where(col(tw < 1), np.where(col(back), np.where(col(sub), fs, z3), front_f), z3)
    brdf_pdf = np.where(tw < 1, np.where(back, np.where(sub, ps * s.subsurface * dr, z1), front_p), z1)
    return np.concatenate([mix(brdf, bsdf, col(tw)), col(mix(brdf_pdf, bsdf_pdf, tw))], 1), None


class Draws:
    """rand(seed) of random.glsl:98-102 drawn under a mask: lanes outside the mask keep their state (the number of draws per branch is part of
    the contract).  Records the margin of every `rand() < threshold` comparison."""

    def __init__(self, seed, ft):
        self.s, self.ft, self.margin = seed.copy(), ft, np.full(len(seed), np.inf)

    def rand(self, mask=None):
        s2, w = pcg_step(self.s)
        if mask is None:
            self.s = s2
        else:
            self.s = np.where(mask, s2, self.s)
        return word_to_float(w).astype(self.ft)

    def less(self, thr, mask):
        r = self.rand(mask)
        with np.errstate(invalid="ignore"):
            m = np.abs(r.astype(np.float64) - thr.astype(np.float64))
        self.margin = np.where(mask, np.minimum(self.margin, np.where(np.isnan(m), 0.0, m)), self.margin)
        return mask & (r < thr)


def select(branch, parts, width):
    out = np.zeros((len(branch), width), parts[0].dtype)
    for k, p in enumerate(parts):
        out = np.where(col(branch == k), p, out)
    return out


DISNEY_BRANCHES = ["reflection", "refraction", "subsurface", "diffuse", "specular", "clearcoat"]


def disney_sample(rows, ft):  # :414-520
    s = state_of(rows, ft)
    V, N = s.V, s.N
    n = len(V)
    all_, z1 = np.ones(n, bool), np.zeros(n, ft)
    d = Draws(s.seed, ft)
    r1, r2 = d.rand(), d.rand()
    dr, tw = ft(0.5) * (ft(1) - s.metallic), (ft(1) - s.metallic) * s.transmission
    psr = ft(1) / (ft(1) + s.clearcoat)
    trans = d.less(tw, all_)
    with np.errstate(all="ignore"):
        # BSDF
        H = to_world(s, sample_gtr2(s.roughness, r1, r2))
        R = reflect(-V, H)
        F = dielectric_fresnel(np.abs(dot(R, H)), s.eta)
        F = np.where(s.thin & s.back, ft(0), F)  # :442-446
        eta = np.where(s.thin, ft(1.001), s.eta)
        refl = d.less(F, trans)
        L0 = normalize(R)
        f0, p0 = d_reflection(s, eta, V, N, L0, H, z1)
        L1 = normalize(refract(-V, H, eta))
        f1, p1 = d_refraction(s, eta, V, N, L1, H)
        # BRDF
        brdf = ~trans
        diff = d.less(dr, brdf)
        subs = d.less(s.subsurface, diff)
        L2 = to_world(s, uniform_hemisphere(r1, r2), -1)
        f2, p2 = d_subsurface(s, V, N, L2)
        p2 = p2 * s.subsurface * dr
        L3 = to_world(s, cosine_hemisphere(r1, r2))
        f3, p3 = d_diffuse(s, s.sheenTint, V, N, L3, normalize(L3 + V), z1)
        p3 = p3 * (ft(1) - s.subsurface) * dr
        spec = brdf & ~diff
        prim = d.less(psr, spec)
        H4 = to_world(s, sample_gtr2_aniso(s.ax, s.ay, r1, r2))
        L4 = normalize(reflect(-V, H4))
        f4, p4 = d_specular(s, d_spec_tint(s), V, N, L4, H4, z1)
        p4 = p4 * psr * (ft(1) - dr)
        H5 = to_world(s, sample_gtr1(s.clearcoatRoughness, r1, r2))
        L5 = normalize(reflect(-V, H5))
        f5, p5 = d_clearcoat(s, V, N, L5, H5, z1)
        p5 = p5 * (ft(1) - psr) * (ft(1) - dr)
    branch = np.where(trans, np.where(refl, 0, 1), np.where(diff, np.where(subs, 2, 3), np.where(prim, 4, 5)))
    w = np.where(trans, tw, ft(1) - tw)
    L = select(branch, [L0, L1, L2, L3, L4, L5], 3)
    f = select(branch, [f0, f1, f2, f3, f4, f5], 3) * col(w)
    pdf = select(branch, [col(p) for p in (p0, p1, p2, p3, p4, p5)], 1)[:, 0] * w
    return np.concatenate([L, f, col(pdf)], 1), (d.s, branch, d.margin)


# ---- shaders/pbr_gltf.glsl ----------------------------------------------------------------------------------------------------------------------
def f_schlick(f0, f90, vdh):  # :39-47
    return f0 + (f90 - f0) * clamp(vdh.dtype.type(1) - vdh, 0, 1) ** vdh.dtype.type(5)


def v_ggx(ndl, ndv, a):  # :54-67
    ft = ndl.dtype.type
    a2 = a * a
    g = ndl * np.sqrt(ndv * ndv * (ft(1) - a2) + a2) + ndv * np.sqrt(ndl * ndl * (ft(1) - a2) + a2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g > 0, ft(0.5) / g, ft(0))


def v_ggx_aniso(ndl, ndv, bdv, tdv, tdl, bdl, at, ab):  # :71-77
    gv = ndl * np.sqrt((at * tdv) ** 2 + (ab * bdv) ** 2 + ndv ** 2)
    gl = ndv * np.sqrt((at * tdl) ** 2 + (ab * bdl) ** 2 + ndl ** 2)
    return clamp(ndl.dtype.type(0.5) / (gv + gl), 0, 1)


def d_ggx(ndh, a):  # :98-103
    ft = ndh.dtype.type
    a2 = a * a
    f = (ndh * ndh) * (a2 - ft(1)) + ft(1)
    return a2 / (ft(PI) * f * f)


def d_ggx_aniso(ndh, tdh, bdh, at, ab):  # :108-114
    a2 = at * ab
    w2 = a2 / ((ab * tdh) ** 2 + (at * bdh) ** 2 + (a2 * ndh) ** 2)
    return a2 * w2 * w2 / ndh.dtype.type(PI)


def g_f0_f90(s):  # :412-415 == :502-505
    refl = np.maximum(np.maximum(s.f0[:, 0], s.f0[:, 1]), s.f0[:, 2])
    return s.f0, col(clamp(refl * s.ft(50), 0, 1)) * np.ones((1, 3), s.ft)


def g_diffuse(s, V, N, L):  # :204-220 + BRDF_lambertian :132-138
    ft = s.ft
    ndl, ndv = dot(N, L), dot(N, V)
    off = (ndl < 0) | (ndv < 0)
    pdf = clamp(ndl, 0.001, 1) * ft(1 / PI)
    return np.where(col(off), ft(0), col(ft(1) - s.metallic) * (s.albedo / ft(PI))), np.where(off, ft(0), pdf)


def g_specular(s, f0, f90, V, N, L, H):  # :225-284 + :141-176
    ft = s.ft
    ndl0 = dot(N, L)
    off = ndl0 < 0
    ndl, ndv = clamp(ndl0, 0.001, 1), clamp(np.abs(dot(N, V)), 0.001, 1)
    # anisotropic (:225-258, :151-176)
    tdv, bdv = clamp(dot(s.T, V), 0, 1), clamp(dot(s.B, V), 0, 1)
    tdl, bdl, tdh, bdh, ndh, vdh, ldh = dot(s.T, L), dot(s.B, L), dot(s.T, H), dot(s.B, H), dot(N, H), dot(V, H), dot(L, H)
    at, ab = np.maximum(s.roughness * (ft(1) + s.anisotropy), ft(0.001)), np.maximum(s.roughness * (ft(1) - s.anisotropy), ft(0.001))
    pa = d_ggx_aniso(ndh, tdh, bdh, at, ab) / (ft(4) * ldh)
    at2, ab2 = np.maximum(s.roughness * (ft(1) + s.anisotropy), ft(0.00001)), np.maximum(s.roughness * (ft(1) - s.anisotropy), ft(0.00001))
    fa = f_schlick(f0, f90, col(vdh)) * col(v_ggx_aniso(ndl, ndv, bdv, tdv, tdl, bdl, at2, ab2) * d_ggx_aniso(ndh, tdh, bdh, at2, ab2))
    # isotropic (:262-284, :141-148)
    ndh_c, ldh_c, vdh_c = clamp(ndh, 0, 1), clamp(ldh, 0, 1), clamp(vdh, 0, 1)
    pi_ = d_ggx(ndh_c, s.roughness) * ndh_c / (ft(4) * ldh_c)
    fi = f_schlick(f0, f90, col(vdh_c)) * col(v_ggx(ndl, ndv, s.roughness) * d_ggx(ndh_c, np.maximum(ft(0.001), s.roughness)))
    an = s.anisotropy > 0
    return np.where(col(off), ft(0), np.where(col(an), fa, fi)), np.where(off, ft(0), np.where(an, pa, pi_))


def g_clearcoat(s, V, N, L, H):  # :289-314
    ft = s.ft
    ndl0 = dot(N, L)
    off = ndl0 < 0
    ndh, vdh, ldh = dot(N, H), dot(V, H), dot(L, H)
    ndl, ndv = clamp(ndl0, 0.001, 1), clamp(np.abs(dot(N, V)), 0.001, 1)
    F = f_schlick(ft(0.04), ft(1), vdh)
    a = s.clearcoatRoughness * s.clearcoatRoughness
    G, D = v_ggx(ndl, ndv, a), d_ggx(ndh, np.maximum(ft(0.001), a))
    pdf = D * ndh / (ft(4) * ldh)
    return np.where(col(off), ft(0), col(F * D * G * s.clearcoat) * np.ones((1, 3), ft)), np.where(off, ft(0), pdf)


def gltf_eval(rows, ft):  # :365-434
    s = state_of(rows, ft)
    V, N, L = s.V, s.N, s.L
    z1, z3 = np.zeros(len(s.V), ft), np.zeros((len(s.V), 3), ft)
    with np.errstate(all="ignore"):
        H = half_vector(s, V, N, L)
        dr, psr, tw = ft(0.5) * (ft(1) - s.metallic), ft(1) / (ft(1) + s.clearcoat), (ft(1) - s.metallic) * s.transmission
        sr = ft(1) - dr
        bsdf = np.where(col(tw > 0), s.albedo, z3)  # EvalDielectricRefractionGltf :340-343
        bsdf_pdf = np.where(tw > 0, np.abs(dot(N, L)), z1)
        f0, f90 = g_f0_f90(s)
        fd, pd = g_diffuse(s, V, N, L)
        fc, pc = g_clearcoat(s, V, N, L, H)
        fs, ps = g_specular(s, f0, f90, V, N, L, H)
        on = (tw < 1) & (dot(N, L) > 0)
        brdf = np.where(col(on), (fd + fc) + fs, z3)
        brdf_pdf = np.where(on, (pd * dr + pc * (ft(1) - psr) * sr) + ps * psr * sr, z1)
    return np.concatenate([mix(brdf, bsdf, col(tw)), col(mix(brdf_pdf, bsdf_pdf, tw))], 1), None


GLTF_BRANCHES = ["transmission-reflect", "transmission-refract", "diffuse", "specular(roughness)", "clearcoat(roughness)", "specular(clearcoatRoughness)",
                 "clearcoat(clearcoatRoughness)"]


def gltf_sample(rows, ft):  # :439-554
    s = state_of(rows, ft)
    V, N = s.V, s.N
    n = len(V)
    all_ = np.ones(n, bool)
    d = Draws(s.seed, ft)
    prob = d.rand()
    dr, tw = ft(0.5) * (ft(1) - s.metallic), (ft(1) - s.metallic) * s.transmission
    sr = ft(1) - dr
    r1, r2 = d.rand(), d.rand()
    trans = d.less(tw, all_)
    with np.errstate(all="ignore"):
        R0 = (ft(1) - s.ior) / (ft(1) + s.ior)
        H = to_world(s, sample_gtr2(s.roughness, r1, r2, floor=False))
        vdh = dot(V, H)
        F = f_schlick(R0 * R0, ft(1), vdh)
        disc = ft(1) - s.eta * s.eta * (ft(1) - vdh * vdh)
        inside = s.thin & s.back  # :466-474
        F, disc = np.where(inside, ft(0), F), np.where(inside, ft(0), disc)
        eta = np.where(s.thin, ft(1), s.eta)
        tir = trans & (disc < 0)  # `discriminat < 0.0 || rand(seed) < F`: no draw behind a true left operand
        d.margin = np.where(trans, np.minimum(d.margin, np.abs(disc.astype(np.float64))), d.margin)
        refl = tir | d.less(F, trans & ~tir)
        L0 = normalize(reflect(-V, H))
        L1 = normalize(refract(-V, H, eta))
        L1 = np.where(col(np.isnan(L1).any(1)), -V, L1)
        f01 = s.albedo
        # BRDF
        f0, f90 = g_f0_f90(s)
        brdf = ~trans
        diff = brdf & (prob < dr)
        d.margin = np.where(brdf, np.minimum(d.margin, np.abs(prob.astype(np.float64) - dr.astype(np.float64))), d.margin)
        L2 = to_world(s, cosine_hemisphere(r1, r2))
        f2, p2 = g_diffuse(s, V, N, L2)
        p2 = p2 * (ft(1) - s.subsurface) * dr
        spec = brdf & ~diff
        psr = ft(1) / (ft(1) + s.clearcoat)
        own = d.less(psr, spec)
        prim = d.less(psr, spec)
        res = []
        for rough in (s.roughness, s.clearcoatRoughness):
            Hs = to_world(s, sample_gtr2(rough, r1, r2, floor=False))
            Ls = reflect(-V, Hs)
            fs, ps = g_specular(s, f0, f90, V, N, Ls, Hs)
            fc, pc = g_clearcoat(s, V, N, Ls, Hs)
            res += [(Ls, fs * col(ft(1) - tw), ps * psr * sr * (ft(1) - tw)), (Ls, fc * col(ft(1) - tw), pc * (ft(1) - psr) * sr * (ft(1) - tw))]
    branch = np.where(trans, np.where(refl, 0, 1), np.where(diff, 2, np.where(own, np.where(prim, 3, 4), np.where(prim, 5, 6))))
    L = select(branch, [L0, L1, L2] + [r[0] for r in res], 3)
    f = select(branch, [f01, f01, f2 * col(ft(1) - tw)] + [r[1] for r in res], 3)
    pdf = select(branch, [col(np.abs(dot(N, L0))), col(np.abs(dot(N, L1))), col(p2 * (ft(1) - tw))] + [col(r[2]) for r in res], 1)[:, 0]
    return np.concatenate([L, f, col(pdf)], 1), (d.s, branch, d.margin)


# ---- the built-ins as probe rows -----------------------------------------------------------------------------------------------------------------
def k_reflect(x, ft):
    x = x.astype(ft)
    return reflect(x[:, 0:3], x[:, 3:6])


def k_refract(x, ft):
    x = x.astype(ft)
    return refract(x[:, 0:3], x[:, 3:6], x[:, 6])


def k_mix(x, ft):
    x = x.astype(ft)
    return mix(x[:, 0:3], x[:, 3:6], col(x[:, 6]))


def k_smoothstep(x, ft):
    x = x.astype(ft)
    with np.errstate(divide="ignore", invalid="ignore"):
        return col(smoothstep(x[:, 0], x[:, 1], x[:, 2]))


# the scalar built-ins, rows (a, b, c): GLSL 4.60 specification 8.1 (atan) and 8.3
def k_scalar(which):
    def f(x, ft):
        x = x.astype(ft)
        a, b, c = x[:, 0], x[:, 1], x[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = {"step": lambda: np.where(b < a, ft(0), ft(1)),            # 0.0 if x < edge, otherwise 1.0
                 "clamp": lambda: np.minimum(np.maximum(a, b), c),         # min(max(x, minVal), maxVal)
                 "sign": lambda: np.where(a > 0, ft(1), np.where(a < 0, ft(-1), ft(0))),  # 1, 0 or -1 (0 for both zeros)
                 "fract": lambda: a - np.floor(a),                         # x - floor(x)
                 "mod": lambda: a - b * np.floor(a / b),                   # x - y floor(x / y)
                 "atan": lambda: np.arctan2(a, b),                         # atan(y, x): the angle whose tangent is y / x, quadrant from the signs, in [-pi, pi]
                 "roundEven": lambda: np.rint(a)}[which]()                 # nearest integer, .5 to the nearest even one
        return col(r)
    return f


def scalar_inputs():
    g = Stream(400, 6)
    u = lambda lo, hi: g.u(lo, hi)  # noqa: E731
    z = np.zeros(400)
    rows = lambda a, b=z, c=z, e=(): np.concatenate([np.stack([a, b, c], 1), np.array([list(r) + [0] * (3 - len(r)) for r in e], np.float64).reshape(-1, 3)]).astype(np.float32)  # noqa: E731
    out = []
    e = [(0.5, 0.5), (0.5, 0.49999997), (0.5, 0.50000006), (0.0, -0.0), (-1.0, -1.0)]
    out.append(("step", rows(u(-1, 1), u(-1, 1), e=e), [f"edge, x = {r}" for r in e]))
    lo = u(-1, 0.5)
    e = [(0.25, 0.25, 0.75), (0.75, 0.25, 0.75), (-3, 0, 1), (3, 0, 1), (0.5, 0, 1)]
    out.append(("clamp", rows(u(-2, 2), lo, lo + u(0, 1), e=e), [f"x, lo, hi = {r}" for r in e]))
    e = [(0.0,), (-0.0,), (1e-38,), (-1e-38,), (3.0,), (-3.0,)]
    out.append(("sign", rows(u(-2, 2), e=e), ["+0", "-0", "+1e-38", "-1e-38", "3", "-3"]))
    e = [(-0.25,), (-1.0,), (2.0,), (0.75,), (-3.5,), (1e6 + 0.5,)]
    out.append(("fract", rows(u(-10, 10), e=e), [f"x = {r[0]}" for r in e]))
    sgn = np.where(g.u() < 0.5, -1.0, 1.0)
    e = [(-1, 3), (1, -3), (5.5, -2), (-5.5, 2), (6, 3), (-6, 3), (0.5, 1), (-0.5, 1)]
    out.append(("mod", rows(u(-10, 10), sgn * u(0.5, 4), e=e), [f"x, y = {r}" for r in e]))
    e = [(0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1), (-0.0, -1)]
    out.append(("atan", rows(u(-2, 2), u(-2, 2), e=e), [f"y, x = {r}" for r in e]))
    e = [(0.5,), (1.5,), (2.5,), (-0.5,), (-1.5,), (-2.5,), (0.49999997,), (2.5000002,), (8388609.0,)]
    out.append(("roundEven", rows(u(-20, 20), e=e), [f"x = {r[0]}" for r in e]))
    return out


SCALARS = ["step", "clamp", "sign", "fract", "mod", "atan", "roundEven"]


# ---- vector and matrix built-ins as the shaders use them (GLSL 4.60 specification 5.10, 8.5): matrices are column-major, m[c][r] ---------------------
def k_cross(x, ft):
    x = x.astype(ft)
    return cross(x[:, 0:3], x[:, 3:6])


def k_normalize(x, ft):  # x / length(x)
    with np.errstate(all="ignore"):
        return normalize(x.astype(ft))


def columns(x, rows_per_col, ncol):
    return [x[:, rows_per_col * k:rows_per_col * (k + 1)] for k in range(ncol)]


def k_mat4_vec4(x, ft):  # M * v = sum over columns c of M[c] v[c]   (camera rays: pathtrace.comp / pathtrace.glsl viewInverse * vec4, projInverse * vec4)
    x = x.astype(ft)
    return sum(c * col(x[:, 16 + k]) for k, c in enumerate(columns(x, 4, 4)))


def k_vec4_mat4(x, ft):  # v * M: component c = dot(v, M[c])
    x = x.astype(ft)
    return np.stack([dot(x[:, 16:20], c) for c in columns(x, 4, 4)], 1)


def k_xform_point(x, ft):  # mat4x3 M * vec4(p, 1)   (shade_state.glsl: objectToWorld * vec4(pos, 1))
    x = x.astype(ft)
    c = columns(x, 3, 4)
    return c[0] * col(x[:, 12]) + c[1] * col(x[:, 13]) + c[2] * col(x[:, 14]) + c[3]


def k_xform_dir(x, ft):  # mat4(M) * vec4(d, 0)
    x = x.astype(ft)
    c = columns(x, 3, 4)
    return c[0] * col(x[:, 12]) + c[1] * col(x[:, 13]) + c[2] * col(x[:, 14])


def k_xform_rowvec(x, ft):  # vec3(n * M): component c = dot(n, M[c])   (shade_state.glsl: normal * worldToObject)
    x = x.astype(ft)
    return np.stack([dot(x[:, 12:15], c) for c in columns(x, 3, 3)], 1)


def k_mat3_vec3(x, ft):  # mat3(c0, c1, c2) * v   (gltf_material.glsl:116 TBN)
    x = x.astype(ft)
    c = columns(x, 3, 3)
    return c[0] * col(x[:, 9]) + c[1] * col(x[:, 10]) + c[2] * col(x[:, 11])


def matrix_inputs():
    """(name, function, rows, names of the hand-made rows).  Hand-made: a matrix of distinct integers against the unit vectors -- exact, and different for
    every mix-up of rows and columns; a pure translation."""
    g = Stream(200, 8)
    rnd = lambda k: np.stack([g.u(-2, 2) for _ in range(k)], 1)  # noqa: E731
    out = []
    e = [[1, 0, 0, 0, 1, 0], [0, 1, 0, 1, 0, 0], [1, 2, 3, 1, 2, 3], [1, 2, 3, -2, 0.5, 4]]
    out.append(("cross", k_cross, np.concatenate([rnd(6), e]).astype(np.float32), ["x cross y = z", "y cross x = -z", "parallel", "general"]))
    e = [[3, 4, 0], [0, 0, -2], [1e-3, 0, 0], [1e-20, 0, 0], [1, 1, 1]]
    out.append(("normalize", k_normalize, np.concatenate([rnd(3), e]).astype(np.float32), ["3 4 0", "axis", "short", "dot underflows in float32", "diagonal"]))
    m4 = list(range(1, 17))
    e4 = [m4 + list(v) for v in ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 2, 3, 4])]
    n4 = ["distinct integers, e0", "e1", "e2", "e3", "v = 1 2 3 4"]
    out.append(("mat4_vec4", k_mat4_vec4, np.concatenate([rnd(20), e4]).astype(np.float32), n4))
    out.append(("vec4_mat4", k_vec4_mat4, np.concatenate([rnd(20), e4]).astype(np.float32), n4))
    m3 = list(range(1, 13))
    e3 = [m3 + list(v) for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 2, 3])] + [[1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 6, 7, 1, 2, 3]]
    n3 = ["distinct integers, e0", "e1", "e2", "p = 1 2 3", "pure translation"]
    for name, fn in (("xform_point", k_xform_point), ("xform_rowvec", k_xform_rowvec), ("xform_dir", k_xform_dir)):
        out.append((name, fn, np.concatenate([rnd(15), e3]).astype(np.float32), n3))
    e = [list(range(1, 10)) + list(v) for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 2, 3])]
    out.append(("mat3_vec3", k_mat3_vec3, np.concatenate([rnd(12), e]).astype(np.float32), ["distinct integers, e0", "e1", "e2", "v = 1 2 3"]))
    return out


# ---- shaders/env_sampling.glsl:38-99 Environment_sample ------------------------------------------------------------------------------------------------
ENV_W, ENV_H = 2, 4  # rows 0 and 3 touch the poles
ENV_BRANCHES = ["texel", "alias"]


def env_table():
    """a hand-made EnvAccel table (alias, q, pdf, aliasPdf per texel): every pdf value is different, so the pdf returned names the texel and the choice"""
    alias = np.array([3, 0, 5, 1, 7, 2, 0, 4], np.uint32)
    q = np.array([0.25, 1.0, 0.5, 0.75, 0.125, 0.9, 0.6, 1.0], np.float32)
    k = np.arange(8, dtype=np.float32)
    t = np.zeros((8, 4), np.float32)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = alias.view(np.float32), q, np.float32(0.1) + k / np.float32(64), np.float32(0.5) + k / np.float32(64)
    return t


def env_sample(rows, ft):
    n = len(rows)
    xi = rows[:, 0:3].astype(ft)
    w, h = rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int64)
    tab = rows[:, 8:40].reshape(n, 8, 4)
    size = w * h
    idx = np.minimum((xi[:, 0] * size.astype(ft)).astype(np.int64), size - 1)          # :46-47
    pick = np.arange(n)
    alias = np.ascontiguousarray(tab[pick, idx, 0]).view(np.uint32).astype(np.int64)
    q, p_own, p_alias = tab[pick, idx, 1].astype(ft), tab[pick, idx, 2].astype(ft), tab[pick, idx, 3].astype(ft)
    own = xi[:, 1] < q                                                                     # :57-72
    with np.errstate(all="ignore"):
        y = np.where(own, xi[:, 1] / q, (xi[:, 1] - q) / (ft(1) - q))
    env_idx = np.where(own, idx, alias)
    pdf = np.where(own, p_own, p_alias)
    px, py = env_idx % w, env_idx // w                                                     # :75-76
    u = (px.astype(ft) + y) / w.astype(ft)                                                 # :80
    phi = u * ft(2 * PI) - ft(PI)
    step = ft(PI) / h.astype(ft)                                                           # :85-90
    theta0 = py.astype(ft) * step
    cos_theta = np.cos(theta0) * (ft(1) - xi[:, 2]) + np.cos(theta0 + step) * xi[:, 2]
    with np.errstate(invalid="ignore"):
        theta = np.arccos(cos_theta)
    sin_theta = np.sin(theta)
    v = theta * ft(1 / PI)
    out = np.stack([np.cos(phi) * sin_theta, cos_theta, np.sin(phi) * sin_theta, pdf, u, v], 1)   # :93
    margin = np.abs(xi[:, 1].astype(np.float64) - q.astype(np.float64))
    return out, (env_idx.astype(np.uint32), (~own).astype(np.int64), margin)


def env_inputs():
    g = Stream(600, 9)
    xi = np.stack([g.u(), g.u(), g.u()], 1)
    below1 = float(np.float32(1) - np.float32(2.0 ** -24))
    e, names = [], []
    for k, qv in enumerate(env_table()[:, 1]):
        for side, dy in (("below", -1e-3), ("above", 1e-3)):
            if qv + dy < 1:
                e.append([(k + 0.5) / 8, qv + dy, 0.5]); names.append(f"texel {k}, xi.y just {side} q")
    for nm, x in (("xi.x = 0 (first texel, first row)", 0.0), ("xi.x just below 1 (last texel, last row)", below1)):
        for nz, z in (("xi.z = 0", 0.0), ("xi.z = 0.5", 0.5), ("xi.z just below 1", below1)):
            e.append([x, 0.05, z]); names.append(f"{nm}, {nz}")
    e.append([0.3, 0.0, 0.3]); names.append("xi.y = 0")
    e.append([0.3, below1, 0.3]); names.append("xi.y just below 1")
    xi = np.concatenate([xi, e])
    rows = np.zeros((len(xi), 40), np.float32)
    rows[:, 0:3], rows[:, 3], rows[:, 4] = xi, ENV_W, ENV_H
    rows[:, 8:40] = env_table().reshape(-1)
    return rows, names


# ---- shaders/env_sampling.glsl:111-125: the light direction EnvSample picks under Sun & Sky.  Rows: the 24 words of SunAndSky (host_device.h:258-281:
# sun_direction = words 16-18, sun_disk_scale = word 19), then the RNG state -----------------------------------------------------------------------------
def sun_disk(rows, ft):
    sd = rows[:, 16:19].astype(ft)
    radius = ft(np.float32(0.00465) * np.float32(10.0)) * rows[:, 19].astype(ft)             # :116
    tb = coordinate_system(rows[:, 16:19], ft)                                               # :117-118
    d = Draws(np.ascontiguousarray(rows[:, 24]).view(np.uint32), ft)
    x = d.rand() * radius                                                                    # :120-122
    y = d.rand() * radius
    z = np.sqrt(np.maximum(ft(0), ft(1) - x * x - y * y))
    with np.errstate(all="ignore"):
        light = normalize(tb[:, 0:3] * col(x) + tb[:, 3:6] * col(y) + sd * col(z))           # :124
    return np.concatenate([light, np.full((len(rows), 1), 0.5, ft)], 1), (d.s, np.zeros(len(rows), np.int64), d.margin)   # :126 pdf = 0.5


def sun_disk_inputs():
    g = Stream(400, 14)
    sd = g.unit()
    scale = 10.0 ** g.u(-1, 1)
    e = [([0, 1, 0], 1.0), ([0, -1, 0], 1.0), ([0, 0, 1], 1.0), ([0, 0, -1], 4.0), ([0.9363, 0.1, 0.3366], 0.0), ([0.9363, 0.1, 0.3366], 30.0)]
    names = ["sun at +y", "sun at -y", "sun at +z (the other tangent branch)", "sun at -z, scale 4", "sun_disk_scale 0", "sun_disk_scale 30 (x^2 + y^2 can exceed 1: z = 0)"]
    sd = np.concatenate([sd, [a for a, _ in e]])
    scale = np.concatenate([scale, [b for _, b in e]])
    rows = np.zeros((len(sd), 25), np.float32)
    rows[:, 16:19], rows[:, 19] = f32_unit(sd), scale
    rows[:, 23] = np.array([1], np.int32).view(np.float32)[0]   # in_use
    rows[:, 24] = Stream(len(sd), 15).word().view(np.float32)
    return rows, names


# ---- shaders/tonemapping.glsl:29-105: rows rgb[3] exposure ----------------------------------------------------------------------------------------------
def t_linear_to_srgb(c):  # :29-32
    return c ** c.dtype.type(1 / 2.2)


def t_srgb_to_linear(c):  # :36-39
    return c ** c.dtype.type(2.2)


def t_uncharted_impl(c):  # :48-57
    ft = c.dtype.type
    A, B, C, D, E, F = ft(0.15), ft(0.50), ft(0.10), ft(0.20), ft(0.02), ft(0.30)
    return ((c * (A * c + C * B) + D * E) / (c * (A * c + B) + D * F)) - E / F


def t_uncharted(c):  # :59-65
    ft = c.dtype.type
    white = ft(1) / t_uncharted_impl(np.full((1, 3), 11.2, c.dtype))
    return t_linear_to_srgb(t_uncharted_impl(c * ft(2)) * white)


def t_hejl_richard(c):  # :69-73
    ft = c.dtype.type
    c = np.maximum(ft(0), c - ft(0.004))
    return (c * (ft(6.2) * c + ft(0.5))) / (c * (ft(6.2) * c + ft(1.7)) + ft(0.06))


def t_aces(c):  # :77-85
    ft = c.dtype.type
    A, B, C, D, E = ft(2.51), ft(0.03), ft(2.43), ft(0.59), ft(0.14)
    return t_linear_to_srgb(clamp((c * (A * c + B)) / (c * (C * c + D) + E), 0, 1))


TONEMAPS = {"linearTosRGB": t_linear_to_srgb, "sRGBToLinear": t_srgb_to_linear, "toneMapUncharted": t_uncharted, "toneMapHejlRichard": t_hejl_richard, "toneMapACES": t_aces,
            "toneMap": None}  # :88-105 with TONEMAP_UNCHARTED (post.frag:30): toneMapUncharted(color * exposure)


def k_tonemap(which):
    def f(x, ft):
        x = x.astype(ft)
        with np.errstate(all="ignore"):
            return t_uncharted(x[:, 0:3] * col(x[:, 3])) if which == "toneMap" else TONEMAPS[which](x[:, 0:3])
    return f


def tonemap_inputs():
    g = Stream(400, 10)
    # (log-uniform from 1e-2: below that the Uncharted curve's "- E / F" cancels against its quotient in float32 itself; the small values stay as an edge row)
    rgb = np.stack([10.0 ** g.u(-2, 2) for _ in range(3)], 1)
    e = [[0, 0, 0, 1], [1e-4, 1e-3, 1e-2, 1], [1, 1, 1, 1], [11.2, 11.2, 11.2, 1], [5.6, 5.6, 5.6, 1], [1e4, 1e4, 1e4, 1], [0.004, 0.0039, 0.0041, 1], [0.5, 0.25, 0.125, 4.0]]
    names = ["0", "small values", "1", "the Uncharted white point", "half the white point (Uncharted doubles its input)", "1e4", "around Hejl-Richard's 0.004", "exposure 4"]
    return np.concatenate([np.concatenate([rgb, col(g.u(0.25, 4))], 1), e]).astype(np.float32), names


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def derived(m):
    """ax, ay (gltf_material.glsl:118-121) and f0 (:123-124) of a material vector, in float32 like the loader computes them"""
    m = m.astype(np.float32)
    aspect = np.sqrt(np.float32(1) - m[:, 4] * np.float32(0.9))
    m[:, 17] = np.maximum(np.float32(0.001), m[:, 6] / aspect)
    m[:, 18] = np.maximum(np.float32(0.001), m[:, 6] * aspect)
    dsp = ((m[:, 16] - 1) / (m[:, 16] + 1)) ** 2
    m[:, 19:22] = col(dsp * (1 - m[:, 5])) + m[:, 0:3] * col(m[:, 5])
    return m


def frame(N, t):
    N = f32_unit(N)
    T = f32_unit(np.cross(N, f32_unit(t)))
    return N, T, np.cross(N, T).astype(np.float32)


def bsdf_grid(n, salt, sampling=False):
    """random shading states reaching every lobe of both BSDFs: the generator idea of tests/test_oracle_vs_ref.py bsdf_inputs on the pinned stream.
    Roughly 15 % have dot(N, V) <= 0 (outside the model's domain: stored, never kept).

    sampling: the distribution for the sample functions.  A sampled half vector sits on the peak of its lobe, where float32 itself is ill-conditioned
    for three input classes that the evaluation grid has in bulk (measured with the model alone, float32 against float64):
      roughness 0.001          1 + (a^2 - 1) NdotH^2 cancels to ~1e-6                   -> roughness and clearcoatRoughness from [0.1, 1), the extreme stays in the edge list
      thin-walled (eta 1.001)  LdotH eta + VdotH of the refraction lobe cancels to ~1e-3 -> 2 % of the states instead of 25 %
      ior 1.0 / clearcoatRoughness 1   the shader divides 0 by 0 (refraction denominator, ImportanceSampleGTR1): NaN as written -> edge list only
    (and subsurface and clearcoat are never exactly 0 there, so that their branches are reached often enough.)
    They all stay in the grids of the evaluation functions, and every stored state is compared bit for bit between the builds."""
    g = Stream(n, salt)

    def pick(*opts):
        k = g.u()
        return np.where(k < 0.5, opts[0], opts[1]) if len(opts) == 2 else np.select([k < 1 / 3, k < 2 / 3], opts[:2], opts[2])

    m = np.zeros((n, 22))
    m[:, 0:3] = np.stack([g.u(0.02, 1) for _ in range(3)], 1)
    m[:, 3] = 0.5
    m[:, 4] = pick(0.0, g.u(0, 0.95))
    m[:, 5] = pick(0.0, 1.0, g.u())
    m[:, 6] = pick(g.u(0.1, 1), g.u(0.1, 1), 1.0) if sampling else np.maximum(0.001, pick(g.u(), 0.001, 1.0))
    m[:, 7] = g.u() if sampling else pick(0.0, g.u())
    m[:, 8] = g.u()
    m[:, 9] = pick(0.0, g.u())
    m[:, 10:13] = np.stack([g.u() for _ in range(3)], 1)
    m[:, 13] = g.u() if sampling else pick(0.0, g.u())
    m[:, 14] = g.u(0.1, 0.95) if sampling else np.maximum(0.001, pick(g.u(), g.u(), 1.0))
    m[:, 15] = pick(0.0, 1.0, g.u())
    m[:, 16] = pick(1.5, 1.3, g.u(1.05, 2.4)) if sampling else pick(1.5, 1.0, g.u(1.05, 2.4))
    m = derived(m)
    N, T, B = frame(g.unit(), g.unit())
    V, L = f32_unit(g.unit()), f32_unit(g.unit())
    flip = (g.u() < 0.85) & ((V * N).sum(1) < 0)
    V = np.where(col(flip), -V, V)
    inside = g.u() < 0.3
    eta = np.where(inside, m[:, 16], np.float32(1) / m[:, 16]).astype(np.float32)
    thin = (g.u() < (0.02 if sampling else 0.25)).astype(np.float32)
    rows = np.zeros((n, 40), np.float32)
    rows[:, 0:22], rows[:, 22:25], rows[:, 25:28], rows[:, 28:31], rows[:, 31], rows[:, 32], rows[:, 33:36], rows[:, 36:39] = m, N, T, B, eta, thin, V, L
    rows[:, 39] = g.word().view(np.float32)
    return rows


EDGE_SEEDS = 8


def bsdf_edges():
    """named edge states, each with EDGE_SEEDS different RNG states"""
    base = np.zeros(22)
    base[0:3], base[3], base[6], base[8], base[10:13], base[14], base[16] = (0.8, 0.6, 0.4), 0.5, 0.5, 0.5, 0.5, 0.5, 1.5
    n0 = np.array([0.36, 0.48, 0.8])
    t0 = np.array([0.8, -0.6, 0.0])
    b0 = np.cross(n0, t0)

    def at(cos, az=0.7):  # unit vector at dot(N, .) = cos
        sn = np.sqrt(1 - cos * cos)
        return n0 * cos + (t0 * np.cos(az) + b0 * np.sin(az)) * sn

    V0, L0 = at(0.8), at(0.6, 2.5)
    out = []

    def add(name, V=V0, L=L0, eta=1 / 1.5, thin=0, **kw):
        m = base.copy()
        idx = dict(albedo=slice(0, 3), anisotropy=4, metallic=5, roughness=6, subsurface=7, sheen=9, clearcoat=13, clearcoatRoughness=14, transmission=15, ior=16)
        for k, v in kw.items():
            m[idx[k]] = v
        out.append((name, m, V, L, eta, thin))

    add("normal incidence", V=n0, L=n0, clearcoat=0.5, sheen=0.5)
    add("dot(N,L) = +1e-3", L=at(1e-3, 2.5), clearcoat=0.5)
    add("dot(N,L) = -1e-3", L=at(-1e-3, 2.5), transmission=0.5, subsurface=0.5)
    add("roughness 0.001", roughness=0.001)
    add("roughness 1", roughness=1.0, anisotropy=0.5)
    add("clearcoatRoughness 1 (GTR1 branch)", clearcoat=1.0, clearcoatRoughness=1.0)
    add("metallic 0", sheen=1.0, subsurface=0.3)
    add("metallic 1", metallic=1.0)
    add("transmission 1 from outside", L=at(-0.7, 2.5), transmission=1.0)
    add("transmission 1 from inside", L=at(-0.9, 2.5), V=at(0.95), transmission=1.0, eta=1.5)
    add("ior 1.0 (f0 = 0)", ior=1.0, eta=1.0, transmission=0.5)
    add("thin-walled from outside", L=at(-0.7, 2.5), transmission=1.0, thin=1)
    add("thin-walled from inside", L=at(-0.7, 2.5), transmission=1.0, thin=1, eta=1.5)
    add("total internal reflection", V=at(0.2), L=at(0.2, 0.7 + np.pi), transmission=1.0, eta=1.5, roughness=0.05)
    add("black albedo (Cdlum == 0)", albedo=0.0, clearcoat=0.3)
    names, rows = [], []
    for name, m, V, L, eta, thin in out:
        for k in range(EDGE_SEEDS):
            r = np.zeros(40, np.float32)
            r[0:22] = derived(m[None])[0]
            r[22:25], r[25:28], r[28:31], r[31], r[32], r[33:36], r[36:39] = n0, t0, b0, eta, thin, V, L
            names.append(f"{name} #{k}")
            rows.append(r)
    rows = np.array(rows, np.float32)
    rows[:, 39] = Stream(len(rows), 77).word().view(np.float32)
    return names, rows


def vec_grid(n, salt, extra):
    return np.concatenate([f32_unit(Stream(n, salt).unit()), np.array(extra, np.float32)]).astype(np.float32)


AXES = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]


def sky_dirs():
    """the 1508 directions of the sun & sky probes (gen_sky_kat.py builds its sphere class from them)"""
    return vec_grid(1500, 13, AXES + [[0.70710678, 0.70710678, 0], [0, -0.70710678, -0.70710678]])


def simple_inputs():
    """(name, function, rows, names of the hand-made rows at the end)"""
    # (unit-vector outputs -- the tangent frame, reflect / refract of a unit vector -- are compared by absolute error like the sampled L: a component
    # near zero is the difference of O(1) products: N_ABS below)
    g = Stream(400, 5)
    out = []
    diag = [[0.70710678, 0.70710678, 0], [0, -0.70710678, -0.70710678], [0.70710678, 0, -0.70710678], [-0.70710678, 0, 0.70710678]]
    out.append(("spherical_uv", spherical_uv, vec_grid(600, 11, AXES + diag), [f"axis {a}" for a in AXES] + [f"diagonal {a}" for a in diag]))
    out.append(("coordinate_system", coordinate_system, vec_grid(600, 12, AXES + [[0.001, 0.002, 0.999998], [0.003, 0.0, -0.9999955]]),
                [f"N = {a}" for a in AXES] + ["just inside the |N.z| > 0.99999 branch", "just outside the |N.z| > 0.99999 branch"]))
    rng_ = np.where(g.u() < 1 / 3, -1.0, np.where(g.u() < 0.5, 0.0, g.u(0.1, 50)))
    ra = np.stack([rng_, g.u(0.01, 60)], 1)
    ra_edge = [[10, 10], [10, 20], [10, 1e-3], [0, 5], [-1, 5], [50, 49.999]]
    out.append(("range_attenuation", range_attenuation, np.concatenate([ra, ra_edge]).astype(np.float32), [f"range, distance = {e}" for e in ra_edge]))
    p2l, sd = g.unit() * col(g.u(0.1, 20)), g.unit() * col(g.u(0.1, 3))
    oc = g.u(-1, 1)
    ic = oc + (1 - oc) * g.u()
    sp = np.concatenate([p2l, sd, col(oc), col(ic)], 1)
    sp_edge = [[0, 0, -2, 0, 0, 1, 0.5, 0.8], [0, -1, -1, 0, 0, 1, 0.5, 0.9], [0, -3, -1, 0, 0, 1, 0.5, 0.9], [0, -1, -1, 0, 0, 1, 0.70710678, 0.9], [1, 0, 0, 1, 0, 0, -1, 1]]
    out.append(("spot_attenuation", spot_attenuation, np.concatenate([sp, sp_edge]).astype(np.float32),
                ["on the axis (1)", "inside the blend", "outside the cone (0)", "at the outer edge", "pointing away, widest cone"]))
    a, b = g.unit(), g.unit()
    rf_edge = [[1, 0, 0, 0, 1, 0], [0, -1, 0, 0, 1, 0], [0.6, -0.8, 0, 0, 1, 0], [0.6, -0.8, 0, 0, -1, 0]]
    out.append(("reflect", k_reflect, np.concatenate([np.concatenate([a, b], 1), rf_edge]).astype(np.float32),
                ["I perpendicular to N", "I = -N", "45-ish degrees", "N on the far side (same result)"]))
    I = f32_unit(g.unit()).astype(np.float64)
    Nn = -np.sign(dot(I, b))[:, None] * b
    eta = np.where(g.u() < 0.5, g.u(0.4, 1.0), g.u(1.0, 2.4))
    rr_edge = [[1, 0, 0, 0, 1, 0, 1.0], [0.6, -0.8, 0, 0, 1, 0, 1.5], [0.6, -0.8, 0, 0, 1, 0, 1 / 1.5], [0.98, -0.19899748, 0, 0, 1, 0, 1.5], [0, -1, 0, 0, 1, 0, 1.5],
               [0.6, -0.8, 0, 0, 1, 0, 1.0], [0.8, -0.6, 0, 0, 1, 0, 1.25]]
    out.append(("refract", k_refract, np.concatenate([np.concatenate([I, Nn, col(eta)], 1), rr_edge]).astype(np.float32),
                ["k == 0 exactly (I perpendicular to N, eta 1)", "into the denser side", "into the thinner side", "k < 0: zero vector", "normal incidence", "eta 1: straight through",
                 "k == 0 boundary (sin = 0.8, eta 1.25)"]))
    x, y = np.stack([g.u(0, 2) for _ in range(3)], 1), np.stack([g.u(0, 2) for _ in range(3)], 1)
    mx_edge = [[1, 2, 3, 4, 5, 6, 0], [1, 2, 3, 4, 5, 6, 1], [1, 2, 3, 4, 5, 6, -0.5], [1, 2, 3, 4, 5, 6, 1.5], [1, 2, 3, 4, 5, 6, 0.25]]
    out.append(("mix", k_mix, np.concatenate([np.concatenate([x, y, col(g.u())], 1), mx_edge]).astype(np.float32), [f"t = {e[6]}" for e in mx_edge]))
    e0 = g.u(-1, 1)
    e1 = e0 + g.u(0.05, 2)
    ss_edge = [[0, 1, 0], [0, 1, 1], [0, 1, -1], [0, 1, 2], [0, 1, 0.5], [0.5, 0.9, 0.5], [0.5, 0.9, 0.9], [1, 0, 0.25]]
    out.append(("smoothstep", k_smoothstep, np.concatenate([np.stack([e0, e1, e0 + (e1 - e0) * g.u(-0.5, 1.5)], 1), ss_edge]).astype(np.float32),
                [f"edge0, edge1, x = {e}" for e in ss_edge]))
    return out


# ---- conditioning filter + minting -------------------------------------------------------------------------------------------------------------
def measure(got, want, n_abs=0):
    """worst of |got - want| / (|want| + 1e-6) over the outputs of a state; the first n_abs columns (a unit vector) by absolute error.
    NaN where either side is not finite."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / (np.abs(want) + 1e-6)
        e[:, :n_abs] = np.abs(got - want)[:, :n_abs]
    e = np.where(np.isfinite(got) & np.isfinite(want), e, np.nan)
    return np.where(np.isnan(e).any(1), np.nan, np.nanmax(np.where(np.isnan(e), 0, e), 1))


def mint(name, fn, rows, n_abs=0, domain=None, hand=(), branches=None, in_key=None):
    with np.errstate(all="ignore"):
        want, aux64 = fn(rows, np.float64)
        got32, aux32 = fn(rows, np.float32)
    spread = measure(got32, want, n_abs)
    with np.errstate(invalid="ignore"):
        ok = spread <= SPREAD
    reason = np.where(np.isnan(spread), "non-finite expectation", "float32 and float64 evaluation of the model differ by more than SPREAD")
    if aux64 is not None:
        same = (aux64[1] == aux32[1]) & (aux64[0] == aux32[0])
        margin = (aux64[2] >= SPREAD) & (aux32[2] >= SPREAD)
        reason = np.where(ok & ~(same & margin), "a rand() < threshold comparison has a margin below SPREAD", reason)
        ok &= same & margin
    domain = np.ones(len(rows), bool) if domain is None else domain
    kept = ok & domain
    out = {in_key or f"{name}_in": rows, f"{name}_want": want, f"{name}_kept": kept, f"{name}_domain": domain}
    nh = len(hand)
    hand_kept = kept[len(rows) - nh:] if nh else np.zeros(0, bool)
    out[f"{name}_edge_names"] = np.array(list(hand), dtype="U80")
    out[f"{name}_edge_dropped"] = np.array([f"{h}: {r}" for h, k, r in zip(hand, hand_kept, reason[len(rows) - nh:]) if not k], dtype="U200")
    gen = domain.copy()
    gen[len(rows) - nh:] = False  # the cap is about the generated states; hand-made ones are kept or named
    dropped = int((gen & ~kept).sum())
    out[f"{name}_counts"] = np.array([int(gen.sum()), dropped], np.int64)
    assert dropped <= 0.02 * gen.sum(), f"{name}: {dropped} of {gen.sum()} generated states dropped (cap 2 %)"
    if aux64 is not None:
        out[f"{name}_seed_after"], out[f"{name}_branch"] = aux64[0], aux64[1].astype(np.int32)
        per = np.array([int((kept & (aux64[1] == k)).sum()) for k in range(len(branches))], np.int64)
        out[f"{name}_branch_kept"] = per
        out[f"{name}_branch_names"] = np.array(branches, dtype="U40")
        assert (per >= 50).all(), f"{name}: kept states per branch {dict(zip(branches, per))} (at least 50 each)"
    print(f"{name:18s} {len(rows):5d} states, {int(gen.sum()):5d} generated in domain, {dropped:3d} dropped ({100.0 * dropped / max(1, gen.sum()):.2f} %), "
          f"{int((~hand_kept).sum())} of {nh} hand-made dropped" + (f", kept per branch {out[name + '_branch_kept'].tolist()}" if aux64 is not None else ""))
    return out


N_ABS = {"coordinate_system": 6, "reflect": 3, "refract": 3}


def wrap(fn):
    return lambda rows, ft: (fn(rows, ft), None)


def main(path=None):
    out = {"SPREAD": np.float64(SPREAD)}
    for k, v in N_ABS.items():
        out[f"{k}_n_abs"] = np.int64(v)
    names, edges = bsdf_edges()
    grids = {False: np.concatenate([bsdf_grid(N_BSDF, 20), edges]), True: np.concatenate([bsdf_grid(N_BSDF, 21, sampling=True), edges])}
    for name, fn, n_abs, br in (("disney_eval", disney_eval, 0, None), ("gltf_eval", gltf_eval, 0, None), ("disney_sample", disney_sample, 3, DISNEY_BRANCHES),
                                ("gltf_sample", gltf_sample, 3, GLTF_BRANCHES)):
        rows = grids[br is not None]  # one grid for the two evaluation functions, one for the two sample functions
        domain = (rows[:, 22:25].astype(np.float64) * rows[:, 33:36]).sum(1) > 0
        out.update(mint(name, fn, rows, n_abs, domain, names, br, in_key="bsdf_sample_in" if br else "bsdf_eval_in"))
    for name, fn, rows, hand in simple_inputs():
        out.update(mint(name, wrap(fn), rows, N_ABS.get(name, 0), None, hand))
    for name, rows, hand in scalar_inputs():
        out.update(mint(name, wrap(k_scalar(name)), rows, 0, None, hand))
    for name, fn, rows, hand in matrix_inputs():   # sums of O(1) products: absolute error, like the unit vectors
        out[f"{name}_n_abs"] = np.int64(4)
        out.update(mint(name, wrap(fn), rows, 4, None, hand))
    rows, hand = env_inputs()
    out.update(mint("env_sample", env_sample, rows, 3, None, hand, ENV_BRANCHES))
    out["env_sample_texel"] = out.pop("env_sample_seed_after")   # the integer output here: the texel picked
    rows, hand = sun_disk_inputs()
    out.update(mint("sun_disk", sun_disk, rows, 3, None, hand, ["sun disk"]))
    rows, hand = tonemap_inputs()
    for name in TONEMAPS:
        out.update(mint(name, wrap(k_tonemap(name)), rows, 0, None, hand, in_key="tonemap_in"))
    out["sky_dirs"] = sky_dirs()
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "float_kat.npz")
    with zipfile.ZipFile(path, "w") as z:  # like np.savez_compressed, with a fixed timestamp: the same bytes on every run
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

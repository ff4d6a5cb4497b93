"""Mints the DISPLAY known answers in tests/golden/display_kat.npz: an independent float64 model of the display pass and of its mip chain.

The display pass is where Vulkan supplies the most and the reference's own sources pin the least: the vkCmdBlitImage(VK_FILTER_LINEAR) mip chain, the
NEAREST / NEAREST / REPEAT sampler with its level selection and the float -> UNORM8 store are all rules of the Vulkan specification, restated once in
oracle/ref_glue/, once in the oracle and once in the kernels.  This file is the leg that shares nothing with them: numpy only, written from the shader text
(shaders/post.frag, file:line cited per function) and from the Vulkan 1.3 specification (section cited by name per rule), importing nothing of oracle/,
vk_raytrace_amd/ or tests/orc.py.  From gen_float_kat.py it takes what is literally the same rule: the tonemap curves of shaders/tonemapping.glsl, the GLSL
built-ins mix / clamp, the error measure and the pinned PCG stream the inputs are drawn from; from gen_kat.py pcg3d (shaders/random.glsl:81-92).

Every function takes the scalar type from its input, so the same code runs in np.float64 (the expectation) and in np.float32 (only to judge conditioning).

What is modelled
  blit        "Image Copies with Scaling" (vkCmdBlitImage), whole level to whole level: the centre of a destination texel (x + 0.5) is scaled into source
              space by the extent ratio sw / dw -- kept as the exact rational ((2x + 1) sw - dw) / (2 dw) -- and the source is sampled with unnormalised
              coordinates, VK_FILTER_LINEAR ("Texel Filtering": i0 = floor(u - 0.5), alpha = frac(u - 0.5), the weighted sum
              (1-a)(1-b) t00 + a(1-b) t10 + (1-a)b t01 + ab t11) and clamp-to-edge ("Wrapping Operation").
  chain       nvvk::cmdGenerateMipmaps as RenderOutput::genMipmap calls it (src/render_output.cpp:188-193): floor(log2(max(w, h))) + 1 levels ("Image
              Miplevel Sizing": each extent max(1, e / 2)), level i blitted from level i - 1; generated only when autoExposure & 1
              (src/sample_example.cpp:423-427).
  viewport    while the viewer de-scales, the render sits in the top-left corner of a viewport-sized image (src/sample_example.cpp:410-413); texels outside
              are zero, alpha included (the project's choice -- the reference keeps stale data there), and the chain is built from that padded image.
  sampler     the zeroed VkSamplerCreateInfo of src/render_output.cpp:98-100 with maxLod = FLT_MAX: magFilter = minFilter = NEAREST ("Texel Coordinate
              Systems": unnormalised u = s * width, i = floor(u)), addressMode REPEAT ("Wrapping Operation": i mod size), mipmapMode NEAREST.
              Level: "Scale Factor Operation, LOD Operation and Image Level(s) Selection".  The full-screen triangle interpolates uvCoords linearly, and
              post.frag samples at uvCoords * tm.zoom, so ds/dx = zoom / W, dt/dy = zoom / H and the cross terms are 0: rho_x = rho_y = zoom texels of level 0
              per pixel, lambda_base = log2(rho_max / eta) = log2(zoom) (eta = 1, no anisotropy).  lambda' = lambda_base + clamp(samplerBias + shaderBias, ..)
              with samplerBias = 0; lambda = clamp(lambda', minLod = 0, maxLod = FLT_MAX); d' = baseMipLevel + clamp(lambda, 0, levelCount - 1);
              the level is nearest(d') = ceil(d' + 0.5) - 1.  texture(s, uv) has shaderBias 0, texture(s, uv, b) has shaderBias b -- the third argument of
              GLSL's texture() is a BIAS, not a LOD -- and textureLod(s, uv, l) sets lambda' = l.
  post.frag   main :98-147: toneExposure :64-70, toneLocalExposure :72-96 (the loop index at which it breaks is recorded: 0..6, or 7 for "did not break"),
              toneMap (tonemapping.glsl:88-105 with TONEMAP_UNCHARTED, post.frag:30), dither :48-54 on pcg3d(uvec3(gl_FragCoord.xy, 0)) :120 with the noise
              bit trick :128, contrast :135, brightness :137, saturation :139-140, vignette with renderingRatio :142-143, alpha pass-through :146.
              RGB2XYZ :58 is a column-major mat3 constructor (GLSL 5.4.2), so (RGB2XYZ * RGB).y = 0.3575761 R + 0.7151522 G + 0.1191920 B.
  store       "Conversion from Floating-Point to Normalized Fixed-Point": clamp to [0, 1], scale by 2^8 - 1, convert to the nearest integer; 0.0 and 1.0 are
              stored exactly.  The specification does not say what a NaN stores; this model states that it stores 0 (what Direct3D's rule says and what the
              GPUs the reference runs on do), and that min / max / clamp carry a NaN through (IEEE 754 minimum / maximum), so a NaN anywhere in a pixel's
              path reaches the store as NaN.

Kept-pixel rule, decided by the model alone (the rule of gen_float_kat.py): a pixel of a run is KEPT when the model's float32 evaluation of fragColor is
within SPREAD of its float64 evaluation in the measure |a - b| / (|b| + 1e-6) (or both are NaN in the same channels), both evaluations take the same decisions,
and every decision on the pixel's path has a margin of at least SPREAD in both:
  texel choice      |u - nearest integer| / (|u| + 1e-6) for u = s * width of every fetch (a fetch whose u is that close to a texel boundary may land on either side)
  mip level choice  |frac(d') - 0.5| (per run: it does not depend on the pixel; asserted, not filtered)
  break test        | |v1 - v2| / (..) - epsilon |, an ABSOLUTE margin: the quotient's absolute error is bounded by the sum of the relative errors of v1 and v2
                    (the denominator exceeds v1), so it is compared with SPREAD itself, not with SPREAD * epsilon
  dither            floor(s): |s - nearest integer| / (|s| + 1e-6); discr < lin: |discr - lin| / (|lin| + 1e-6)
  final rounding    t = clamp(v, 0, 1) * 255: |t - (floor(t) + 0.5)| / (t + 1e-6), all four channels
A pixel that fails ONLY the final-rounding margin is flagged `round_only`: the tests hold its codes to within 1.  SPREAD is the project's 1e-5; the depth of
this chain did not need another value: the worst float32-to-float64 spread of the model over the pixels it keeps is printed by main() (8.2e-6).
Caps asserted here and again by the test: at most 5 % of a case's pixels dropped, over all its images (round_only ones count as dropped); every local-exposure exit -- break at
i = 0..6 and "no break" -- keeps at least 50 pixels over the fixture.

Edge runs (named; stored and compared between the legs bit for bit, held to the model where the model keeps them): a black pixel under each exposure mode
(hdr / XYZ.y is 0 / 0 under auto-exposure), NaN, +Inf and -Inf pixels alone and under auto-exposure (the chain's 1x1 level goes NaN, so every pixel does, and
all colour codes are 0), an all-black image, a pixel at 3e38 (float32 overflows where float64 does not: never kept).

Run:  python tests/golden/gen_display_kat.py   (rewrites display_kat.npz; deterministic)
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_float_kat import SPREAD, Stream, clamp, mix, t_linear_to_srgb, t_srgb_to_linear, t_uncharted  # noqa: E402
from gen_kat import pcg3d  # noqa: E402

CAP = 0.05
MIN_PER_EXIT = 50
NO_BREAK = 7

# RenderOutput::m_tonemapper (src/render_output.hpp:37-49)
TM_FIELDS = ["brightness", "contrast", "saturation", "vignette", "avgLum", "zoom", "renderingRatio0", "renderingRatio1", "autoExposure", "Ywhite", "key", "dither"]
TM_DEFAULT = dict(brightness=1.0, contrast=1.0, saturation=1.0, vignette=0.0, avgLum=1.0, zoom=1.0, renderingRatio0=1.0, renderingRatio1=1.0, autoExposure=0, Ywhite=0.5,
                  key=0.5, dither=1)
# the seven TM_CASES of tests/test_oracle_vs_ref.py first (tests/test_display_model.py asserts they are these), then the cases of this fixture
CASES = [
    ("tm0", dict()),
    ("tm1", dict(dither=1)),
    ("tm2", dict(autoExposure=1)),
    ("tm3", dict(autoExposure=3)),
    ("tm4", dict(autoExposure=3, key=0.3, Ywhite=2.0, dither=1)),
    ("tm5", dict(brightness=1.4, contrast=1.3, saturation=0.6, vignette=0.5, avgLum=2.0)),
    ("tm6", dict(autoExposure=1, renderingRatio0=0.8, renderingRatio1=0.6, vignette=0.3)),
    ("plain", dict(dither=0)),
    ("ae2", dict(autoExposure=2, dither=0)),  # bit 1 without bit 0: post.frag:103 tests bit 0 first, so this is "plain"
    ("bc_dither", dict(brightness=0.8, contrast=1.2, dither=1)),
    ("vignette_neg", dict(vignette=3.0, dither=0)),  # 1 - dot(uv, uv) * 3 is negative outside the centre: negative colours reach the store
    ("global", dict(autoExposure=1, dither=0)),
    ("local", dict(autoExposure=3, dither=0)),
]
CASE_NAMES = [n for n, _ in CASES]


def tonemapper(over, zoom=1.0):
    tm = dict(TM_DEFAULT, **over)
    tm["zoom"] = zoom
    return {k: (int(v) if k in ("autoExposure", "dither") else float(np.float32(v))) for k, v in tm.items()}


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------------
def blit_axis(s, d, ft):
    """source indices and weight of destination texels 0..d-1 along one axis: u = (x + 0.5) s / d, the linear filter reads floor(u - 0.5) and its neighbour"""
    n = (2 * np.arange(d, dtype=np.int64) + 1) * s - d  # u - 0.5 = n / (2 d), an exact rational
    i0 = n // (2 * d)  # floor
    a = ((n - i0 * 2 * d).astype(np.float64) / (2 * d)).astype(ft)  # frac, rounded once
    return np.clip(i0, 0, s - 1), np.clip(i0 + 1, 0, s - 1), a  # clamp-to-edge


def blit(src, dw, dh):
    ft = src.dtype.type
    sh, sw = src.shape[:2]
    x0, x1, a = blit_axis(sw, dw, ft)
    y0, y1, b = blit_axis(sh, dh, ft)
    a, b = a[None, :, None], b[:, None, None]
    t00, t10, t01, t11 = src[y0][:, x0], src[y0][:, x1], src[y1][:, x0], src[y1][:, x1]
    one = ft(1)
    with np.errstate(all="ignore"):
        return (one - a) * (one - b) * t00 + a * (one - b) * t10 + (one - a) * b * t01 + a * b * t11


def level_count(w, h):
    return int(max(w, h)).bit_length()  # floor(log2(max(w, h))) + 1 for positive integers, without a floating-point log


def build_chain(level0):
    chain = [level0]
    for _ in range(level_count(level0.shape[1], level0.shape[0]) - 1):
        h, w = chain[-1].shape[:2]
        chain.append(blit(chain[-1], max(1, w // 2), max(1, h // 2)))
    return chain


def pad_corner(img, dw, dh):
    out = np.zeros((dh, dw, 4), img.dtype)
    out[:img.shape[0], :img.shape[1]] = img
    return out


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------------------
def select_level(zoom, shader_bias, levels, explicit_lod=None):
    """(level, |frac(d') - 0.5|) of texture(s, uv * zoom[, bias]) in the full-screen pass, or of textureLod(s, uv, explicit_lod)"""
    FLT_MAX = 3.4028234663852886e38
    lam = float(explicit_lod) if explicit_lod is not None else float(np.log2(np.float64(zoom))) + float(shader_bias)
    lam = min(max(lam, 0.0), FLT_MAX)  # minLod = 0, maxLod = FLT_MAX
    d = 0.0 + min(max(lam, 0.0), float(levels - 1))  # baseMipLevel = 0, q = levelCount - 1
    level = int(np.ceil(d + 0.5)) - 1
    return level, abs((d - np.floor(d)) - 0.5)


def margin_int(u):
    with np.errstate(invalid="ignore"):
        return np.abs(u - np.rint(u)) / (np.abs(u) + u.dtype.type(1e-6))


def fetch(level, s, t):
    """NEAREST / REPEAT fetch of one level at normalised (s, t) arrays: (texels, margin of the texel choice)"""
    h, w = level.shape[:2]
    ft = level.dtype.type
    u, v = s * ft(w), t * ft(h)
    i, j = np.floor(u).astype(np.int64) % w, np.floor(v).astype(np.int64) % h
    return level[j, i], np.minimum(margin_int(u), margin_int(v))


def luminance(c):  # post.frag:59-62
    ft = c.dtype.type
    return c[..., 0] * ft(0.2126) + c[..., 1] * ft(0.7152) + c[..., 2] * ft(0.0722)


# ---- post.frag ---------------------------------------------------------------------------------------------------------------------------------------------
def shade(chain, tm, forced_exit=None):
    """post.frag main() on every pixel of the viewport chain[0].  Returns fragColor (H, W, 4), the local-exposure exit (H, W) (-1: not run), La (H, W),
    the smallest decision margin (H, W) without the final rounding, the final-rounding margin (H, W), and the decisions (H, W, k) as integers.
    forced_exit (H, W): take this exit of toneLocalExposure instead of evaluating the break test (the tests recover a leg's exit with it)."""
    ft = chain[0].dtype.type
    H, W = chain[0].shape[:2]
    one = ft(1)
    with np.errstate(all="ignore"):
        # passthrough.vert interpolated at the pixel centre: uvCoords = gl_FragCoord.xy / viewport
        uvx = np.broadcast_to(((np.arange(W, dtype=ft) + ft(0.5)) / ft(W))[None, :], (H, W))
        uvy = np.broadcast_to(((np.arange(H, dtype=ft) + ft(0.5)) / ft(H))[:, None], (H, W))
        zx, zy = uvx * ft(tm["zoom"]), uvy * ft(tm["zoom"])
        levels = level_count(W, H)  # the image is created with the full chain; its levels above 0 hold data only when the chain was generated
        lv, lmargin = select_level(tm["zoom"], 0, levels)
        assert lv < len(chain), "texture() without a bias would read a level that was never generated"
        hdr4, margin = fetch(chain[lv], zx, zy)  # :101
        margin = np.minimum(margin, ft(lmargin))
        rgb = hdr4[..., :3]
        exits = np.full((H, W), -1, np.int64)
        La = np.zeros((H, W), ft)
        decisions = []
        if (tm["autoExposure"] >> 0) & 1:  # :103
            lv, _ = select_level(tm["zoom"], 0, levels, explicit_lod=20)  # :105
            avg, _ = fetch(chain[lv], np.full((1, 1), 0.5, ft), np.full((1, 1), 0.5, ft))
            avg_lum = luminance(avg[..., :3])[0, 0]
            XYZy = ft(0.3575761) * rgb[..., 0] + ft(0.7151522) * rgb[..., 1] + ft(0.1191920) * rgb[..., 2]  # :66 / :74
            Y = (ft(tm["key"]) / avg_lum) * XYZy
            if (tm["autoExposure"] >> 1) & 1:  # :107 -> toneLocalExposure :72-96
                factor = ft(tm["key"]) / avg_lum
                epsilon, phi = ft(0.05), ft(2.0)
                active = np.ones((H, W), bool)
                exits[:] = NO_BREAK
                for i in range(7):
                    l1, m1 = select_level(tm["zoom"], i, levels)
                    l2, m2 = select_level(tm["zoom"], i + 1, levels)
                    t1, f1 = fetch(chain[l1], zx, zy)  # :82
                    t2, f2 = fetch(chain[l2], zx, zy)  # :83
                    v1, v2 = luminance(t1[..., :3]) * factor, luminance(t2[..., :3]) * factor
                    scale = ft(2 ** i)
                    lhs = np.abs(v1 - v2) / ((ft(tm["key"]) * ft(2.0) ** phi / (scale * scale)) + v1)  # :84
                    brk = (lhs > epsilon) if forced_exit is None else (forced_exit == i)
                    here = np.minimum(np.minimum(f1, f2), ft(min(m1, m2)))
                    if forced_exit is None:
                        here = np.minimum(here, np.where(np.isnan(lhs), ft(np.inf), np.abs(lhs - epsilon)))
                    margin = np.where(active, np.minimum(margin, here), margin)
                    La = np.where(active, np.where(brk, v1, v2), La)  # :86 / :90
                    exits = np.where(active & brk, i, exits)
                    active = active & ~brk
                Yd = Y / (one + La)  # :92
            else:
                Yd = (Y * (one + Y / (ft(tm["Ywhite"]) * ft(tm["Ywhite"])))) / (one + Y)  # :68
            rgb = rgb / XYZy[..., None] * Yd[..., None]  # :69 / :94
        decisions.append(exits)
        color = t_uncharted(rgb * ft(tm["avgLum"]))  # :114, tonemapping.glsl:88-105
        if tm["dither"] > 0:  # :117
            xy = np.stack([np.broadcast_to(np.arange(W)[None, :], (H, W)), np.broadcast_to(np.arange(H)[:, None], (H, W)), np.zeros((H, W), np.int64)], -1)
            r = pcg3d(xy.reshape(-1, 3)).reshape(H, W, 3)  # :120 uvec3(gl_FragCoord.xy, 0): the fragment's integer coordinates
            noise = ((np.uint32(0x3F800000) | (r >> np.uint32(9))).astype(np.uint32).view(np.float32) - np.float32(1.0)).astype(ft)  # :128 (exact in float32)
            lin = t_srgb_to_linear(color)  # :131
            quant = ft(np.float32(1.0) / np.float32(255.0))
            s = t_linear_to_srgb(lin) / quant  # :50
            c0 = np.floor(s) * quant
            c1 = c0 + quant
            discr = mix(t_srgb_to_linear(c0), t_srgb_to_linear(c1), noise)  # :52
            up = discr < lin  # :53
            color = np.where(up, c1, c0)
            dm = np.minimum(margin_int(s), np.abs(discr - lin) / (np.abs(lin) + ft(1e-6)))
            margin = np.minimum(margin, np.where(np.isnan(dm), ft(np.inf), dm).min(-1))
            decisions += [np.where(np.isnan(s), -1, np.floor(s)).astype(np.int64)[..., k] for k in range(3)] + [up[..., k].astype(np.int64) for k in range(3)]
        color = clamp(mix(np.full_like(color, 0.5), color, ft(tm["contrast"])), 0, 1)  # :135
        color = color ** (one / ft(tm["brightness"]))  # :137
        grey = color[..., 0] * ft(0.299) + color[..., 1] * ft(0.587) + color[..., 2] * ft(0.114)  # :139
        color = mix(np.repeat(grey[..., None], 3, -1), color, ft(tm["saturation"]))  # :140
        vx = ((uvx * ft(tm["renderingRatio0"])) - ft(0.5)) * ft(2.0)  # :142
        vy = ((uvy * ft(tm["renderingRatio1"])) - ft(0.5)) * ft(2.0)
        color = color * (one - (vx * vx + vy * vy) * ft(tm["vignette"]))[..., None]  # :143
        frag = np.concatenate([color, hdr4[..., 3:4]], -1)  # :145-146
        t = clamp(frag, 0, 1) * ft(255)
        rm = np.abs(t - (np.floor(t) + ft(0.5))) / (t + ft(1e-6))
        rmargin = np.where(np.isnan(rm), ft(np.inf), rm).min(-1)
    return frag, exits, La, margin, rmargin, np.stack(decisions, -1)


def unorm8(frag):
    """the store: clamp, scale by 255, nearest integer; NaN stores 0"""
    with np.errstate(invalid="ignore"):
        t = np.clip(np.asarray(frag, np.float64), 0.0, 1.0) * 255.0
    return np.where(np.isnan(t), 0.0, np.rint(t)).astype(np.uint8)


def measure(got, want):
    """|got - want| / (|want| + 1e-6) per pixel, worst channel; 0 where both are NaN, or the same infinity, in a channel; inf where only one is"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / (np.abs(want) + 1e-6)
    e = np.where((np.isnan(got) & np.isnan(want)) | (got == want), 0.0, e)
    return np.where(np.isnan(e), np.inf, e).max(-1)


def evaluate(img32, disp, tm):
    """one run of the model: both evaluations, the kept rule.  img32: (h, w, 4) float32 render; disp: (W, H) viewport"""
    out = {}
    res = {}
    for ft in (np.float64, np.float32):
        level0 = pad_corner(img32.astype(ft), disp[0], disp[1])
        chain = build_chain(level0) if tm["autoExposure"] & 1 else [level0]
        res[ft] = (chain,) + shade(chain, tm)
    chain, frag, exits, La, margin, rmargin, dec = res[np.float64]
    _, frag32, _, _, margin32, rmargin32, dec32 = res[np.float32]
    spread = measure(frag32, frag)
    sound = (spread <= SPREAD) & (dec == dec32).all(-1) & (margin >= SPREAD) & (margin32 >= SPREAD)
    rounding = (rmargin >= SPREAD) & (rmargin32 >= SPREAD)
    out["frag"] = frag.astype(np.float32)
    out["code"] = unorm8(frag)
    out["kept"] = sound & rounding
    out["round_only"] = sound & ~rounding
    out["exit"] = exits.astype(np.int8)
    return out, chain, float(spread[sound].max()) if sound.any() else 0.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------
MASTER_W, MASTER_H = 130, 66


def blocky(g, w, h, scale):
    """one value per scale x scale block of a w x h image, from the stream g"""
    bw, bh = -(-w // scale), -(-h // scale)
    vals = g.u(-1.0, 1.0)[:bw * bh].reshape(bh, bw)
    return np.repeat(np.repeat(vals, scale, 0), scale, 1)[:h, :w]


def master_image():
    """The HDR-like image every input is cut from (130 x 66): a smooth gradient, lognormal texture over about 1e-3 .. 1e2 whose strength rises along x,
    a few bright spots, dark specks, structure at every scale of the chain, and an alpha that is not constant.
    Rows 0..32 hold the strong texture (exits at the first iterations), rows 33..65 are calm with blocks of +-9 % at the scales 4, 8, 16 and 32 (exits at the later
    ones); the two halves of the calm band differ by just under 10 %, so that the 2x1 level against the 1x1 level breaks at i = 6 on one side only."""
    w, h = MASTER_W, MASTER_H
    g = Stream(w * h, 77)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    strength = 0.02 * (2.2 / 0.02) ** (xx / (w - 1))  # lognormal sigma-like: 0.02 at the left edge, 2.2 at the right one
    tex = sum(blocky(g, w, h, s) * a for s, a in ((1, 1.0), (2, 0.7), (4, 0.5)))
    lum = (0.6 + 0.8 * yy / 32.0) * np.exp(strength * tex)  # the gradient runs down the textured band
    calm = np.ones((h, w))
    for k, s in enumerate((4, 8, 16, 32)):
        seg = (xx >= 8 + 30 * k) & (xx < 8 + 30 * k + 22)
        calm = np.where(seg, 1.0 + 0.09 * np.sign(blocky(g, w, h, s)), calm)
    calm = calm * np.where(xx < w / 2, 1.0 + 0.0485, 1.0 - 0.0485) * (1.0 + 0.004 * g.u(-1.0, 1.0).reshape(h, w))
    top = yy < 33
    lum = np.where(top, lum, calm)
    for (sx, sy, v) in ((100, 8, 110.0), (118, 25, 60.0), (61, 15, 35.0)):  # bright spots
        lum[sy, sx] = v
    for (sx, sy, v) in ((90, 4, 1.2e-3), (125, 30, 2.5e-3), (108, 18, 1.0e-3)):  # dark specks
        lum[sy, sx] = v
    for x0 in range(0, w, 8):  # every 8-column strip of the textured band averages like the calm band below it: the coarse levels stay near the calm band's value
        lum[:33, x0:x0 + 8] *= calm[33:, x0:x0 + 8].mean() / lum[:33, x0:x0 + 8].mean()
    for _ in range(4):  # the 2 x 1 level: left = mean (1 + 0.0485), right = mean (1 - 0.0485), so that |v1 - v2| / v1 at i = 6 is 0.046 on the left and 0.051 on the right
        l6 = build_chain(lum[..., None])[6][0, :, 0]
        lum[:, w // 2:] *= (l6[0] / l6[1]) * (1.0 - 0.0485) / (1.0 + 0.0485)
    chroma = np.stack([1.0 + 0.5 * g.u(-1.0, 1.0).reshape(h, w) for _ in range(3)], -1)
    chroma /= (chroma * [0.2126, 0.7152, 0.0722]).sum(-1, keepdims=True)
    img = np.zeros((h, w, 4), np.float32)
    img[..., :3] = (lum[..., None] * chroma).astype(np.float32)
    img[..., 3] = (0.15 + 0.8 * (0.5 + 0.5 * np.sin(xx * 0.37 + yy * 0.23)) * g.u(0.6, 1.0).reshape(h, w)).astype(np.float32)
    return img


def crop(master, w, h, x0=0, y0=0):
    return np.ascontiguousarray(master[y0:y0 + h, x0:x0 + w])


# (name, render w, h, crop origin, viewport W, H, zoom as (numerator, denominator): tm.zoom = float32(n) / float32(d))
IMAGES = [
    ("1x1", 1, 1, (100, 8), 1, 1, (1, 1)), ("1x5", 1, 5, (99, 6), 1, 5, (1, 1)), ("5x1", 5, 1, (98, 8), 5, 1, (1, 1)), ("2x2", 2, 2, (60, 14), 2, 2, (1, 1)),
    ("3x2", 3, 2, (117, 24), 3, 2, (1, 1)), ("5x3", 5, 3, (88, 3), 5, 3, (1, 1)), ("33x17", 33, 17, (90, 20), 33, 17, (1, 1)), ("67x33", 67, 33, (63, 16), 67, 33, (1, 1)),
    ("75x41", 75, 41, (55, 0), 75, 41, (1, 1)), ("64x64", 64, 64, (33, 2), 64, 64, (1, 1)), ("130x66", 130, 66, (0, 0), 130, 66, (1, 1)),
    # the viewer navigating (src/sample_example.cpp:378,410-413): the render in the corner of the viewport, magnified
    ("37x26in75x53", 37, 26, (80, 14), 75, 53, (1, 2)), ("25x17in75x53", 25, 17, (48, 24), 75, 53, (1, 3)),
    # zoom > 1 (the reference never sets it; the sampler's rules do not care): uv * zoom leaves [0, 1), so REPEAT addressing is seen; at 5/4 lambda_base = 0.32
    # still selects level 0, at 2 lambda_base = 1 moves every fetch one level up (with the chain generated: the levels exist)
    ("33x17zoom5:4", 33, 17, (90, 20), 33, 17, (5, 4)), ("33x17zoom2", 33, 17, (90, 20), 33, 17, (2, 1)),
]
SMALL = ["1x1", "1x5", "5x1", "2x2", "3x2", "5x3", "33x17"]
RUNS = [(im, c) for im in SMALL for c in CASE_NAMES] + [("67x33", "tm3"), ("67x33", "local"), ("75x41", "tm5"), ("75x41", "bc_dither"), ("64x64", "tm4"), ("64x64", "local"),
                                                          ("130x66", "local"), ("37x26in75x53", "tm3"), ("25x17in75x53", "local"),
                                                          ("33x17zoom5:4", "plain"), ("33x17zoom5:4", "local"), ("33x17zoom2", "local")]


def edge_runs():
    """(name, image (h, w, 4) float32, case): 3 x 2 images around one special pixel"""
    base = np.array([[[0.8, 0.5, 0.3, 0.91], [1.5, 1.2, 0.7, 0.52], [0.2, 0.3, 0.6, 1.0]], [[0.05, 0.04, 0.03, 0.25], [3.0, 2.0, 4.0, 0.75], [0.6, 0.6, 0.6, 0.0]]], np.float32)
    runs = []
    for mode, case in (("no exposure", "tm0"), ("global exposure", "tm2"), ("local exposure", "tm3")):
        black = base.copy()
        black[0, 1, :3] = 0.0
        runs.append((f"a black pixel, {mode}", black, case))
        runs.append((f"an all-black image, {mode}", np.concatenate([np.zeros((2, 3, 3), np.float32), base[..., 3:]], -1), case))
        for what, v in (("NaN", np.nan), ("+Inf", np.inf), ("-Inf", -np.inf)):
            img = base.copy()
            img[1, 1, :3] = v
            runs.append((f"a {what} pixel, {mode}", img, case))
    big = base.copy()
    big[0, 2, :3] = 3e38
    runs.append(("a pixel at 3e38, no exposure", big, "plain"))
    runs.append(("a pixel at 3e38, global exposure", big, "global"))
    return runs


# ---- minting -----------------------------------------------------------------------------------------------------------------------------------------------
def main(path=None):
    master = master_image()
    cases = dict(CASES)
    out = {"SPREAD": np.float64(SPREAD), "master": master, "case_names": np.array(CASE_NAMES, dtype="U16"), "tm_fields": np.array(TM_FIELDS, dtype="U16"),
           "image_names": np.array([i[0] for i in IMAGES], dtype="U16"), "image_geometry": np.array([[i[1], i[2], i[3][0], i[3][1], i[4], i[5], i[6][0], i[6][1]] for i in IMAGES], np.int64),
           "run_image": np.array([r[0] for r in RUNS], dtype="U16"), "run_case": np.array([r[1] for r in RUNS], dtype="U16")}
    geo = {i[0]: i for i in IMAGES}
    for name, over in CASES:
        tm = tonemapper(over)
        out[f"tm_{name}"] = np.array([tm[k] for k in TM_FIELDS], np.float64)
    per_exit = np.zeros(8, np.int64)
    per_case = {}  # the cap holds per case, over all its images (a 1 x 1 image can only drop 0 % or 100 %; the centre column of an odd width sits on a texel boundary of every coarser level)
    worst = 0.0
    chains = {}
    for k, (im, case) in enumerate(RUNS):
        _, w, h, (x0, y0), W, H, (num, den) = geo[im]
        tm = tonemapper(cases[case], zoom=np.float32(num) / np.float32(den))
        res, chain, spread = evaluate(crop(master, w, h, x0, y0), (W, H), tm)
        worst = max(worst, spread)
        if len(chain) > 1 or level_count(W, H) == 1:
            chains[im] = chain
        for key, v in res.items():
            out[f"run{k}_{key}"] = v
        dropped = int((~res["kept"]).sum())
        out[f"run{k}_counts"] = np.array([W * H, dropped, int(res["round_only"].sum())], np.int64)
        per_case[case] = per_case.get(case, np.zeros(2, np.int64)) + [W * H, dropped]
        if tm["autoExposure"] == 3:
            per_exit += np.bincount(res["exit"][res["kept"]].astype(np.int64), minlength=8)
        print(f"run {k:3d} {im:>13s} {case:12s} {W * H:5d} pixels, {dropped:3d} dropped ({100.0 * dropped / (W * H):.2f} %), {int(res['round_only'].sum())} for the rounding only"
              + (f", exits {np.bincount(res['exit'].ravel().astype(np.int64), minlength=8).tolist()}" if tm["autoExposure"] == 3 else ""))
    # the 'ae2' case must behave as 'plain'
    for k, (im, case) in enumerate(RUNS):
        if case == "ae2":
            j = RUNS.index((im, "plain"))
            assert np.array_equal(out[f"run{k}_frag"], out[f"run{j}_frag"], equal_nan=True), "autoExposure = 2 differs from 0"
    out["exit_kept"] = per_exit
    for case, (n, d) in per_case.items():
        print(f"case {case:12s} {n:6d} pixels, {d:4d} dropped ({100.0 * d / n:.2f} %)")
        assert d <= CAP * n, f"case {case}: {d} of {n} pixels dropped (cap 5 %)"
    out["case_counts"] = np.array([per_case[c] for c in CASE_NAMES], np.int64)
    assert (per_exit >= MIN_PER_EXIT).all(), f"kept pixels per local-exposure exit {per_exit.tolist()} (at least {MIN_PER_EXIT} each)"
    for im in [i[0] for i in IMAGES]:  # the model's chain of every image: float64 rounded to float32 (half an ulp: the tests add it to their bound)
        _, w, h, (x0, y0), W, H, _ = geo[im]
        chain = chains.get(im) or build_chain(pad_corner(crop(master, w, h, x0, y0).astype(np.float64), W, H))
        out[f"chain_{im}_levels"] = np.int64(len(chain))
        for lod in range(1, len(chain)):
            out[f"chain_{im}_{lod}"] = chain[lod].astype(np.float32)
    edges = edge_runs()
    out["edge_names"] = np.array([e[0] for e in edges], dtype="U60")
    out["edge_case"] = np.array([e[2] for e in edges], dtype="U16")
    for k, (name, img, case) in enumerate(edges):
        res, _, _ = evaluate(img, (3, 2), tonemapper(cases[case]))
        out[f"edge{k}_in"] = img
        for key in ("frag", "code", "kept", "round_only"):
            out[f"edge{k}_{key}"] = res[key]
        if "exposure" in name and "no exposure" not in name and ("NaN" in name or "Inf" in name or "all-black" in name):
            assert (res["code"][..., :3] == 0).all(), name  # the 1x1 level is NaN or infinite, so every pixel's exposure is NaN or 0: every colour code is 0
    print(f"kept pixels per local-exposure exit (break at 0..6, no break): {per_exit.tolist()}; worst float32 spread on a sound pixel {worst:.2e}")
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "display_kat.npz")
    with zipfile.ZipFile(path, "w") as z:  # like np.savez_compressed, with a fixed timestamp: the same bytes on every run
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

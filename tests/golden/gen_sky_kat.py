"""Mints tests/golden/sky_kat.npz: the procedural sun & sky held to an INDEPENDENT float64 model, direction by direction.

shaders/sun_and_sky.glsl:31-601 restated in numpy from the shader text (lines cited per function), vectorised over probe rows: the 24 words of SunAndSky
(host_device.h:258-281) and a direction.  It imports numpy, the standard library and the other generators of this directory only; nothing of oracle/,
tests/orc.py, tests/ref.py or vk_raytrace_amd/.  Every function takes the scalar type: np.float64 is the expectation, np.float32 only judges conditioning.
Constants are the float32 values of the shader's literals (GLSL has no double literals without a suffix); M_PI is 3.1415926535f (sun_and_sky.glsl:25-27).
calc_irrad's two `for(float u = 1. / 10.; u < 1.; u += 1. / 5.)` loops run in float32 as written: five values each, the third is exactly 0.5.

Quirks followed as written:
  * xyz2dir's "degenerate transform" retry (:57-67) recomputes the vector it already has; the model computes it once.
  * the middle sample of calc_irrad (u = v = 0.5) takes mi_lib_square_to_disk's "pathological" branch (:80-84): r = 0, straight up.
  * sky_color_xyz's local_saturation is the constant 1 (:212-215).
  * the result is multiplied by M_PI twice: calc_env_color :265 and sun_and_sky :598.  `multiplier <= 0` returns vec3(0) before either (:476-479).
  * tweak_saturation answers 1 for every saturation above 1 (:295-307): a boosted saturation is ignored, haze or not.
  * arch_colortweak's `saturation > 1.0` block clamps its by-value parameter `tint` AFTER out_tint was computed from it (:341-351): no effect.
  * the sky is evaluated on the tweaked direction and sun (z raised to 0.001, renormalised), the sun disc on the untweaked ones (:483-505, :523).
  * night_brightness_adjustment is called for sun.z < 0 only (:499-502): a sun in [0, 0.001) keeps factor 1; it sees the sun after the y_is_up swizzle and
    the horizon shift.  Full night (factor 0) still evaluates calc_sun_color and calc_irrad on the raised sun, then multiplies the ground by 0.
  * calc_sun_color's `sun_dir.z > 0` (:147) is always true: the sun it gets has z >= 0.001.  Its turbidity is 2 for directions at or below the horizon (:520).
  * the ground term uses `data_sun_color * sun_dir.z` with the RAISED sun (:553), and calc_irrad always runs with haze 2 (:552).
  * sun_direction is normalised before the swizzle (:493-495); the default (0, 0.78, 0.62) is not a unit vector.
  * acos(dot(real_dir, real_sun)) (:523) is undefined in GLSL when float32 rounding pushes the dot above 1 -- which happens on the very ray that looks at the
    sun.  Such rows are stored, compared bit for bit between the builds, and never kept.  sky_luminance and sky_color_xyz fold a cosine above 1 back
    (:172-175, :231-234), but with the disc enabled no kept row can reach the fold.
  * pow(x, 3.0) of tweak_saturation is undefined for x < 0 in GLSL; the fixture has no negative saturation.

Rows.  SETTINGS: the six variants of tests/test_oracle_vs_ref.py sunsky_variants (restated here; the test asserts they are the same words) and one hand-made
row per branch no committed sky input reached before.  Directions per settings row:
  sphere    gen_float_kat.sky_dirs(): all 1508, on every settings row
  horizon   BAND directions whose tweaked z lies round 0 and round 0.001: the ground blend, dn > 1, the night colour's max per component
  fan       FAN directions round the tweaked sun, classed by angle / sun_radius and the smoothstep's edges: core (smoothstep 1), rise, glow (smoothstep 0),
            rim (0.95 - 1.05 radii) and outside; the core of a physically scaled sun is a class of its own (1 - cos(0.02) cancels in float32)
  sun       the sun direction itself and its float32 neighbours (no cap: most have a float32 dot above 1)

Error measure, stored in the fixture: vector-relative, max over the three channels of |a - b| divided by max over the channels of |b| (0 when both are
all zero).  The channels come out of a 3 x 3 colour matrix with cancelling terms; a channel near zero has no relative accuracy of its own -- the reason
gen_float_kat.py holds its matrix products by absolute error.

Kept mask, by the model alone: the float32 and the float64 evaluation take every branch alike, both results are finite, the measure of one against the
other is within SPREADS[class] (gen_float_kat.SPREAD except where noted there), and the float32 dot(real_dir, real_sun) cannot exceed 1 in any evaluation
order (DOT_MARGIN), and moving every dot(direction, sun) by -+ 2^-23 in the float64 evaluation stays within the same spread (DOT_NUDGE).  EVERY row is stored and compared bit for bit between the builds, kept or not.
Caps, asserted here and again by tests/test_sky_model.py: sphere, horizon, glow, rim, outside at most 2 % dropped; core at least 50 kept rows under a
physically_scaled_sun == 0 setting; core of a physically scaled sun at least 50 kept rows; rise at least 30 kept rows; every branch of BRANCHES at least
50 kept rows.

BREAK: the rules tests/test_sky_model.py's docstring lists as broken one at a time to prove that the check can fail (main(path, brk)).

Run:  python tests/golden/gen_sky_kat.py   (rewrites sky_kat.npz; deterministic, byte-identical on every run)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_float_kat as fk  # noqa: E402
from gen_surface_kat import write_npz  # noqa: E402

MEASURE = "max over channels of |got - want| / max over channels of |want|; 0 where both are all zero"
CLASSES = ("sphere", "horizon", "core", "core, physically scaled", "rise", "glow", "rim", "outside", "sun")
C_SPHERE, C_HORIZON, C_CORE, C_CORE_PHYS, C_RISE, C_GLOW, C_RIM, C_OUTSIDE, C_SUN = range(9)
# the spread of a class: gen_float_kat.SPREAD wherever the class allows it.  Where not (measured with this model alone, float32 against float64):
#   core, physically scaled   every row of a settings row sits at one value up to 2e-4: calc_physical_scale's 1 - cos(sun_disk_radius), radius ~ 0.02, costs
#                             eps / (r^2 / 2) in float32 and scales the whole disc term
#   rise                      acos near 1 has absolute error ~ eps / sin(angle), multiplied by the smoothstep's slope and 100 * sun_disk_intensity * disk_scale
#   glow                      the same acos error through pow(sun_factor / 10, 3) close to the smoothstep's foot: up to 7e-5 inside 0.3 radii
SPREADS = {"sphere": fk.SPREAD, "horizon": fk.SPREAD, "core": fk.SPREAD, "core, physically scaled": 3e-4, "rise": 1e-4, "glow": 1e-4, "rim": fk.SPREAD,
           "outside": fk.SPREAD, "sun": fk.SPREAD}
# "Rows whose float32 dot(real_dir, real_sun) exceeds 1 are never kept" has to hold for EVERY float32 evaluation of that dot, not only numpy's: the legs may
# contract it into fused multiply-adds or sum in another order.  Both vectors are normalised in float32 (length within 1 +- 2^-23 each, so their product
# within 2^-22), and three products and two sums round by at most 2^-24 each of values <= 1: any evaluation is within 2^-22 + 5 * 2^-24 < 2^-21 of the exact
# cosine.  So a row whose float64 cosine is above 1 - 2^-21 (an angle below 1e-3 rad, 0.4 % of the default sun radius) is never kept either.
DOT_MARGIN = 2.0 ** -21
# Conditioning beyond numpy's own float32: the legs' dot and acos may round differently from numpy's, and acos near 1 turns one rounding of the cosine into
# eps / sin(angle) of the angle.  So the float64 model is evaluated twice more with every dot(direction, sun) of the function (the disc's :523, sky_luminance's
# :226, sky_color_xyz's :171) moved by -+ 2^-23, and a row is kept only when both stay within the class's spread: no rounding of that size may matter.
DOT_NUDGE = 2.0 ** -23
DROP_CAPPED = ("sphere", "horizon", "glow", "rim", "outside")
BREAK = ("perez_digit", "zenith_swapped", "xyz2rgb_row", "cos_gamma_fold", "tan_chi", "irrad_16", "y_is_up_ignored", "night_squared_once", "glow_exponent_2",
         "smoothstep_no_haze", "radius_no_10", "target_keeps_max_glow", "dn_unclamped", "redblueshift_sign")
BRANCHES = ("y_is_up 1", "y_is_up 0", "horizon_height != 0", "haze < 0: clamped to 2", "saturation <= 1, haze in (0, 15)", "saturation <= 1, haze above 15: clamped",
            "saturation > 1: tweak answers 1", "luminance(rgb_scale) < 0", "multiplier <= 0", "direction raised to z = 0.001", "direction above 0.001",
            "sun above 0.001", "sun in [0, 0.001): raised, factor 1", "sun in (-0.309, 0): night factor", "sun <= -0.309: full night", "sun_disk_intensity 0",
            "sun_disk_scale 0", "inside the sun radius", "outside the sun radius", "physically scaled", "not physically scaled", "glow integral > max glow",
            "glow integral <= max glow", "smoothstep 0", "smoothstep rising", "smoothstep 1", "cos_gamma < 0", "below the horizon: ground blend", "dn > 1: clamped",
            "dn in (0, 1)", "horizon_blur <= 0", "saturation <= 0: grey", "night colour wins a channel", "night colour loses every channel", "turbidity 2 below the horizon")
BIT = {name: np.uint64(1) << np.uint64(k) for k, name in enumerate(BRANCHES)}

# ---- the settings rows ---------------------------------------------------------------------------------------------------------------------------------------
W_RGB, W_MULT, W_HAZE, W_RBS, W_SAT, W_HH, W_GROUND, W_BLUR, W_NIGHT, W_DISK_I, W_SUN, W_DISK_S, W_GLOW, W_YUP, W_PHYS, W_INUSE = 0, 3, 4, 5, 6, 7, 8, 11, 12, 15, 16, 19, 20, 21, 22, 23
DEFAULT = dict(rgb_unit_conversion=(1, 1, 1), multiplier=0.0000101320, haze=0.0, redblueshift=0.0, saturation=1.0, horizon_height=0.0, ground_color=(0.4, 0.4, 0.4),
               horizon_blur=0.1, night_color=(0.0, 0.0, 0.01), sun_disk_intensity=0.8, sun_direction=(0.00, 0.78, 0.62), sun_disk_scale=5.0, sun_glow_intensity=1.0,
               y_is_up=1, physically_scaled_sun=1, in_use=1)   # src/sample_example.hpp:176-193, in use
SETTINGS = (
    ("variant 0: the defaults", {}),
    ("variant 1: haze 3, redblueshift 0.3, saturation 1.4", dict(haze=3.0, redblueshift=0.3, saturation=1.4)),
    ("variant 2: sun below the horizon", dict(sun_direction=(0.9363, -0.1, 0.3366))),
    ("variant 3: y_is_up 0", dict(y_is_up=0, physically_scaled_sun=1)),
    ("variant 4: horizon_height 0.3, blur 0.5, disc scale 4, glow 2.5", dict(horizon_height=0.3, horizon_blur=0.5, sun_disk_scale=4.0, sun_glow_intensity=2.5)),
    ("variant 5: multiplier 0.25, no disc", dict(multiplier=0.25, sun_disk_intensity=0.0)),
    ("physically_scaled_sun 0, otherwise the defaults", dict(physically_scaled_sun=0)),
    ("glow integral above max glow (disc scale 30, glow 3)", dict(sun_disk_scale=30.0, sun_glow_intensity=3.0)),
    ("saturation 0", dict(saturation=0.0)),
    ("horizon_blur 0", dict(horizon_blur=0.0)),
    ("multiplier 0", dict(multiplier=0.0)),
    ("rgb_unit_conversion negative", dict(rgb_unit_conversion=(-1.0, -1.0, -1.0), multiplier=0.8)),
    ("haze -1", dict(haze=-1.0)),
    ("full night: sun below -0.309", dict(sun_direction=(0.3, -0.8, 0.5))),
    ("sun_disk_scale 0", dict(sun_disk_scale=0.0)),
    ("saturation 1.4 with haze 6", dict(saturation=1.4, haze=6.0, physically_scaled_sun=0)),
    ("saturation 0.6 with haze 8, redblueshift -0.2", dict(saturation=0.6, haze=8.0, redblueshift=-0.2, physically_scaled_sun=0)),
    ("saturation 0.5 with haze 20", dict(saturation=0.5, haze=20.0)),
    ("y_is_up 0, unit sun direction, not physically scaled", dict(y_is_up=0, sun_direction=(0.36, 0.48, 0.8), physically_scaled_sun=0)),
    ("horizon_height 0.5, sun near the horizon", dict(horizon_height=0.5, sun_direction=(0.95, 0.06, 0.3), physically_scaled_sun=0)),
    ("sun just above z = 0.001", dict(sun_direction=(0.8, 0.0012, 0.6), physically_scaled_sun=0)),
    ("sun just below z = 0.001", dict(sun_direction=(0.8, 0.0008, 0.6), physically_scaled_sun=0)),
    ("dusk: sun between 0 and -0.309", dict(sun_direction=(0.8, -0.15, 0.58), physically_scaled_sun=0)),
)


def words_of(changes):
    """the 24 words of a SunAndSky that differs from DEFAULT in `changes`"""
    s = dict(DEFAULT)
    s.update(changes)
    out = np.zeros(24, np.float32)
    iv = out.view(np.int32)
    out[W_RGB:W_RGB + 3], out[W_MULT], out[W_HAZE], out[W_RBS], out[W_SAT], out[W_HH] = s["rgb_unit_conversion"], s["multiplier"], s["haze"], s["redblueshift"], s["saturation"], s["horizon_height"]
    out[W_GROUND:W_GROUND + 3], out[W_BLUR], out[W_NIGHT:W_NIGHT + 3], out[W_DISK_I] = s["ground_color"], s["horizon_blur"], s["night_color"], s["sun_disk_intensity"]
    out[W_SUN:W_SUN + 3], out[W_DISK_S], out[W_GLOW] = s["sun_direction"], s["sun_disk_scale"], s["sun_glow_intensity"]
    iv[W_YUP], iv[W_PHYS], iv[W_INUSE] = s["y_is_up"], s["physically_scaled_sun"], s["in_use"]
    return out


def settings_words():
    return np.array([words_of(kw) for _, kw in SETTINGS], np.float32)


# ---- shaders/sun_and_sky.glsl ----------------------------------------------------------------------------------------------------------------------------------
col, dot, normalize = fk.col, fk.dot, fk.normalize


class Decisions:
    """every `if` of the function in program order, on the rows that reach it (-1 elsewhere): the float32 and the float64 evaluation must agree on all"""

    def __init__(self, n):
        self.n, self.list, self.bits = n, [], np.zeros(n, np.uint64)

    def decide(self, value, mask=None):
        v = np.asarray(value).astype(np.int8)
        self.list.append(v if mask is None else np.where(mask, v, np.int8(-1)))
        return value

    def tag(self, mask, name):
        self.bits = np.where(mask, self.bits | BIT[name], self.bits)


def luminance(rgb, c):  # :31-34
    return c(0.2126) * rgb[:, 0] + c(0.7152) * rgb[:, 1] + c(0.0722) * rgb[:, 2]


def xyz2dir(main, x, y, z):  # :37-71
    zero = np.zeros(len(main), main.dtype)
    u = np.where(col(np.abs(main[:, 0]) < np.abs(main[:, 1])), np.stack([zero, -main[:, 2], main[:, 1]], 1), np.stack([main[:, 2], zero, -main[:, 0]], 1))
    u = normalize(u)
    v = fk.cross(main, u)
    return col(x) * u + col(y) * v + col(z) * main


def square_to_disk(x, y, c):  # :74-115 for one float32 sample pair -> (r, phi) in the scalar type
    ft = type(c(0))
    lx, ly = ft(2) * ft(x) - ft(1), ft(2) * ft(y) - ft(1)
    q = c(3.1415926535) / c(4.0)
    if lx == 0 and ly == 0:
        return ft(0), ft(0), 0
    if lx > -ly:
        if lx > ly:
            return lx, q * (c(1.0) + ly / lx), 1
        return ly, q * (c(3.0) - lx / ly), 2
    if lx < ly:
        return -lx, q * (c(5.0) + ly / lx), 3
    return -ly, q * (c(7.0) - lx / ly), 4


def calc_sun_color(sun, turbidity, c):  # :141-164 (sun.z > 0 always holds for the raised sun)
    ft = sun.dtype.type
    PI = c(3.1415926535)
    ko = np.array([c(12.0), c(8.5), c(0.9)])
    wl = np.array([c(0.610), c(0.550), c(0.470)])
    sol = np.array([c(1.0) * ft(127500) / c(0.9878), c(0.992) * ft(127500) / c(0.9878), c(0.911) * ft(127500) / c(0.9878)])
    with np.errstate(all="ignore"):
        m = c(1.0) / (sun[:, 2] + c(0.15) * np.power(c(93.885) - np.arccos(sun[:, 2]) * ft(180) / PI, c(-1.253)))
        beta = c(0.04608) * turbidity - c(0.04586)
        ta = np.exp(col(-m * beta) * np.power(wl, -c(1.3))[None])
        to = np.exp(col(-m) * ko[None] * c(0.0035))
        tr = np.exp(col(-m * c(0.008735)) * np.power(wl, c(-4.08))[None])
        out = tr * ta * to * sol[None]
    return np.where(col(sun[:, 2] > 0), out, ft(0))


# the Perez coefficients as (slope in turbidity, offset) of A .. E: luminance Y (:240-244), chromaticity x (:194-198) and y (:203-207)
PEREZ_LUM = ((0.178721, -1.463037), (-0.355402, 0.427494), (-0.022669, 5.325056), (0.120647, -2.577052), (-0.066967, 0.370275))
PEREZ_X = ((-0.019257, None), (-0.066513, 0.000818), (-0.000417, 0.212479), (-0.064097, -0.898875), (-0.003251, 0.045178))   # A: - (0.29 - pow(cos_theta_sun, 0.5) * 0.09)
PEREZ_Y = ((-0.016698, -0.260787), (-0.094958, 0.009213), (-0.007928, 0.210230), (-0.044050, -1.653694), (-0.010922, 0.052919))
# zenith chromaticity: rows multiply t2, turbidity, 1; columns multiply ts3, ts2, theta_sun, 1 (:184-189)
ZENITH_X = ((0.001650, -0.003742, 0.002088, 0.0), (-0.029028, 0.063773, -0.032020, 0.003948), (0.116936, -0.211960, 0.060523, 0.258852))
ZENITH_Y = ((0.002759, -0.006105, 0.003162, 0.0), (-0.042149, 0.089701, -0.041536, 0.005158), (0.153467, -0.267568, 0.066698, 0.266881))
XYZ2RGB = ((3.241, -1.537, -0.499), (-0.969, 1.876, 0.042), (0.056, -0.204, 1.057))   # :263-264


def perez(co, cos_theta, gamma, cos_gamma, theta_sun, cos_theta_sun, ft):  # :200-201 == :209-210 == :246-247
    A, B, C, D, E = co
    with np.errstate(all="ignore"):
        return (((ft(1) + A * np.exp(B / cos_theta)) * (ft(1) + C * np.exp(D * gamma) + E * cos_gamma * cos_gamma))
                / ((ft(1) + A * np.exp(B / ft(1))) * (ft(1) + C * np.exp(D * theta_sun) + E * cos_theta_sun * cos_theta_sun)))


def linear(table, T, c):
    return [c(a) * T + c(b) for a, b in table]


def sky_luminance(d, sun, T, c, dec, mask, nudge=0.0):  # :224-250
    ft = d.dtype.type
    cg = dot(sun, d) + ft(nudge)
    neg = cg < 0
    cg = np.where(neg, ft(0), cg)
    over = cg > 1
    cg = np.where(over, c(2.0) - cg, cg)
    if dec is not None:
        dec.decide(neg, mask); dec.decide(over, mask)
        dec.tag(mask & neg, "cos_gamma < 0")
    with np.errstate(all="ignore"):
        return perez(linear(PEREZ_LUM, T, c), d[:, 2], np.arccos(cg), cg, np.arccos(sun[:, 2]), sun[:, 2], ft)


def sky_color_xyz(d, sun, T, lum, c, dec, mask, brk, nudge=0.0):  # :167-221
    ft = d.dtype.type
    cg = dot(sun, d) + ft(nudge)
    over = cg > 1
    if brk != "cos_gamma_fold":
        cg = np.where(over, c(2.0) - cg, cg)
    if dec is not None:
        dec.decide(over, mask)
    with np.errstate(all="ignore"):
        gamma, cts = np.arccos(cg), sun[:, 2]
        ts = np.arccos(cts)
        t2, ts2 = T * T, ts * ts
        ts3 = ts2 * ts

        def zenith(tab):
            rows = [((c(r[0]) * ts3 + c(r[1]) * ts2) + c(r[2]) * ts) + c(r[3]) for r in tab]
            return (rows[0] * t2 + rows[1] * T) + rows[2]

        zx, zy = zenith(ZENITH_X), zenith(ZENITH_Y)
        if brk == "zenith_swapped":
            zx, zy = zy, zx
        co = linear(PEREZ_X[1:], T, c)
        A = c(PEREZ_X[0][0]) * T - (c(0.29) - np.power(cts, c(0.5)) * c(0.09))
        x = perez([A] + co, d[:, 2], gamma, cg, ts, cts, ft)
        tab = PEREZ_Y if brk != "perez_digit" else ((-0.016698, -0.260787), (-0.094958, 0.009213), (-0.007928, 0.210230), (-0.044050, -1.653694), (-0.010922, 0.053919))
        y = perez(linear(tab, T, c), d[:, 2], gamma, cg, ts, cts, ft)
        sat = c(1.0)
        x = zx * ((x * sat) + (c(1.0) - sat))
        y = zy * ((y * sat) + (c(1.0) - sat))
        return np.stack([(x / y) * lum, lum, ((c(1.0) - x - y) / y) * lum], 1)


def calc_env_color(sun, d, T, c, dec=None, mask=None, brk=None, nudge=0.0):  # :253-267
    ft = d.dtype.type
    PI = c(3.1415926535)
    with np.errstate(all="ignore"):
        ts = np.arccos(sun[:, 2])
        chi = (c(4.0) / c(9.0) - T / c(120.0)) * (PI - ft(2) * ts)
        lum = c(1000.0) * ((c(4.0453) * T - c(4.9710)) * (chi if brk == "tan_chi" else np.tan(chi)) - c(0.2155) * T + c(2.4192))
        lum = lum * sky_luminance(d, sun, T, c, dec, mask, nudge)
        X = sky_color_xyz(d, sun, T, lum, c, dec, mask, brk, nudge)
        M = XYZ2RGB if brk != "xyz2rgb_row" else (XYZ2RGB[0], (-0.969, 1.876, 0.142), XYZ2RGB[2])
        rgb = np.stack([c(r[0]) * X[:, 0] + c(r[1]) * X[:, 1] + c(r[2]) * X[:, 2] for r in M], 1)
    return rgb * PI


def calc_irrad(sun, haze, c, brk):  # :269-289 with mi_reflection_dir_diffuse_x :118-138
    ft = sun.dtype.type
    n = len(sun)
    up = np.tile(np.array([ft(0), ft(0), ft(1)]), (n, 1))
    acc = np.zeros((n, 3), sun.dtype)
    path = []
    u = np.float32(1.0) / np.float32(10.0)
    while u < np.float32(1.0):       # the loop variables are float32 in every evaluation: the shader's own
        v = np.float32(1.0) / np.float32(10.0)
        while v < np.float32(1.0):
            r, phi, which = square_to_disk(u, v, c)
            path.append(which)
            x, y = r * np.cos(phi), r * np.sin(phi)
            z2 = c(1.0) - x * x - y * y
            z = np.sqrt(z2) if z2 > 0 else ft(0)
            path.append(int(z2 > 0))
            one = np.ones(n, sun.dtype)
            acc = acc + calc_env_color(sun, xyz2dir(up, one * x, one * y, one * z), haze, c, brk=brk)
            v = np.float32(v + np.float32(1.0) / np.float32(5.0))
        u = np.float32(u + np.float32(1.0) / np.float32(5.0))
    return acc / c(16.0 if brk == "irrad_16" else 25.0), path


def arch_vectortweak(v, yup, horiz, brk=None):  # :311-324
    o = v if brk == "y_is_up_ignored" else np.where(col(yup == 1), v[:, [0, 2, 1]], v)
    shifted = o.copy()
    shifted[:, 2] = shifted[:, 2] - horiz
    with np.errstate(all="ignore"):
        shifted = normalize(shifted)
    return np.where(col(horiz != 0), shifted, o)


def calc_physical_scale(scale, glow_i, disk_i, c, brk):  # :359-438 -> (disc scale, glow scale, glow integral > max glow)
    ft = scale.dtype.type
    PI = c(3.1415926535)
    with np.errstate(all="ignore"):
        disk_r = c(0.00465) * scale
        glow_r = disk_r * c(10.0)
        integral = glow_i * ((c(4.0) * PI) - (c(24.0) * PI) / (glow_r * glow_r) + (c(24.0) * PI) * np.sin(glow_r) / (glow_r * glow_r * glow_r))
        target = disk_i * PI
        max_glow = c(0.5) * target
        capped = integral > max_glow
        glow_scale = np.where(capped, c(1.0) * (max_glow / integral), c(1.0))
        target = np.where(capped, target if brk == "target_keeps_max_glow" else target - max_glow, target - integral)
        area = ft(2) * PI * (ft(1) - np.cos(disk_r))
        target_i = target / area
        actual_integral = c(1.0) * area
        actual_i = disk_i * c(100.0) * actual_integral / area
        return np.where(target_i == 0, ft(0), target_i / actual_i), glow_scale, capped


def real_vectors(words, d, ft):
    """the untweaked-z direction and sun of :463, :493-496 (after the swizzle and the horizon shift): what the sun disc is measured between"""
    c = lambda x: ft(np.float32(x))  # noqa: E731
    w = words.astype(ft)
    yup = np.ascontiguousarray(words).view(np.int32)[:, W_YUP]
    horiz = w[:, W_HH] / c(10.0)
    with np.errstate(all="ignore"):
        return arch_vectortweak(d.astype(ft), yup, horiz), arch_vectortweak(normalize(w[:, W_SUN:W_SUN + 3]), yup, horiz)


def sun_and_sky(words, d, ft, brk=None, nudge=0.0):  # :453-601 -> (result (n, 3), Decisions, the sun angle over the sun radius, dot(real_dir, real_sun))
    n = len(d)
    c = lambda x: ft(np.float32(x))  # noqa: E731
    PI = c(3.1415926535)
    words = np.ascontiguousarray(words, np.float32)
    w, iw = words.astype(ft), words.view(np.int32)
    yup, phys = iw[:, W_YUP], iw[:, W_PHYS]
    dec = Decisions(n)
    all_ = np.ones(n, bool)
    dec.tag(yup == 1, "y_is_up 1"); dec.tag(yup != 1, "y_is_up 0")
    rgb_scale = w[:, W_RGB:W_RGB + 3]
    horiz = w[:, W_HH] / c(10.0)                                                                  # :462
    dec.tag(horiz != 0, "horizon_height != 0")
    dirv = arch_vectortweak(d.astype(ft), yup, horiz, brk)                                        # :463
    haze = c(2.0) + w[:, W_HAZE]                                                                  # :465-469
    low = dec.decide(haze < 2)
    dec.tag(low, "haze < 0: clamped to 2")
    haze = np.where(low, c(2.0), haze)
    sat_in = w[:, W_SAT]                                                                          # tweak_saturation :292-308
    with np.errstate(all="ignore"):
        lowsat = np.power(sat_in, c(3.0))
        h = (haze - c(2.0)) / c(15.0)
        h_neg, h_over = h < 0, h > 1
        h = np.where(h_neg, ft(0), h)
        h = np.where(h_over, ft(1), h)
        h = np.power(h, c(3.0))
        tweaked = (sat_in * (c(1.0) - h)) + lowsat * h
    le1 = dec.decide(sat_in <= 1)
    dec.decide(h_neg, le1); dec.decide(h_over, le1)
    saturation = np.where(le1, tweaked, c(1.0))
    dec.tag(le1 & (h > 0) & ~h_over, "saturation <= 1, haze in (0, 15)")
    dec.tag(le1 & h_over, "saturation <= 1, haze above 15: clamped")
    dec.tag(~le1, "saturation > 1: tweak answers 1")
    neg_lum = dec.decide(luminance(rgb_scale, c) < 0)                                             # :471-474
    dec.tag(neg_lum, "luminance(rgb_scale) < 0")
    rgb_scale = np.where(col(neg_lum), c(1.0) / c(80000.0), rgb_scale)
    rgb_scale = rgb_scale * col(w[:, W_MULT])                                                     # :475
    zero = dec.decide(w[:, W_MULT] <= 0)                                                          # :476-479
    dec.tag(zero, "multiplier <= 0")
    live = ~zero

    downness = dirv[:, 2]                                                                         # :482-490
    real_dir = dirv
    raise_d = dec.decide(dirv[:, 2] < c(0.001), live)
    dec.tag(live & raise_d, "direction raised to z = 0.001"); dec.tag(live & ~raise_d, "direction above 0.001")
    raised = dirv.copy()
    raised[:, 2] = c(0.001)
    with np.errstate(all="ignore"):
        dirv = np.where(col(raise_d), normalize(raised), dirv)
        sun = normalize(w[:, W_SUN:W_SUN + 3])                                                    # :493-496
    sun = arch_vectortweak(sun, yup, horiz, brk)
    real_sun = sun
    raise_s = dec.decide(sun[:, 2] < c(0.001), live)                                              # :497-505
    sun_neg = dec.decide(sun[:, 2] < 0, live & raise_s)
    lmt = c(0.30901699437494742410229341718282)                                                   # night_brightness_adjustment :441-450
    full_night = dec.decide(sun[:, 2] <= -lmt, live & raise_s & sun_neg)
    f = (sun[:, 2] + lmt) / lmt
    f = f * f
    if brk != "night_squared_once":
        f = f * f
    factor = np.where(raise_s & sun_neg, np.where(full_night, ft(0), f), c(1.0))
    dec.tag(live & ~raise_s, "sun above 0.001"); dec.tag(live & raise_s & ~sun_neg, "sun in [0, 0.001): raised, factor 1")
    dec.tag(live & raise_s & sun_neg & ~full_night, "sun in (-0.309, 0): night factor"); dec.tag(live & raise_s & sun_neg & full_night, "sun <= -0.309: full night")
    raised = sun.copy()
    raised[:, 2] = c(0.001)
    with np.errstate(all="ignore"):
        sun = np.where(col(raise_s), normalize(raised), sun)

    lit = dec.decide(factor > 0, live)                                                            # :507-519
    dim = dec.decide(factor < 1, live & lit)
    tint = calc_env_color(sun, dirv, haze, c, dec, live & lit, brk, nudge)
    tint = np.where(col(dim), tint * col(factor), tint)
    tint = np.where(col(lit), tint, ft(0))
    above = dec.decide(downness > 0, live)                                                        # :520
    dec.tag(live & ~above, "turbidity 2 below the horizon")
    sun_color = calc_sun_color(sun, np.where(above, haze, c(2.0)), c)
    disk_i, disk_s, glow_i = w[:, W_DISK_I], w[:, W_DISK_S], w[:, W_GLOW]
    enabled = dec.decide((disk_i > 0) & (disk_s > 0), live)                                       # :521
    dec.tag(live & ~(disk_i > 0), "sun_disk_intensity 0"); dec.tag(live & (disk_i > 0) & ~(disk_s > 0), "sun_disk_scale 0")
    with np.errstate(all="ignore"):
        cos_sun = dot(real_dir, real_sun) + ft(nudge)
        angle = np.arccos(cos_sun)                                                                # :523
        radius = c(0.00465) * disk_s * (c(1.0) if brk == "radius_no_10" else c(10.0))             # :524
        inside = dec.decide(angle < radius, live & enabled)                                       # :525
        inside = live & enabled & inside
        dec.tag(inside, "inside the sun radius"); dec.tag(live & enabled & ~inside, "outside the sun radius")
        scaled = dec.decide(phys == 1, inside)                                                    # :531-536
        ds, gs, capped = calc_physical_scale(disk_s, glow_i, disk_i, c, brk)
        dec.decide(capped, inside & scaled); dec.decide(ds == 0, inside & scaled)
        dec.tag(inside & scaled, "physically scaled"); dec.tag(inside & ~scaled, "not physically scaled")
        dec.tag(inside & scaled & capped, "glow integral > max glow"); dec.tag(inside & scaled & ~capped, "glow integral <= max glow")
        ds, gs = np.where(scaled, ds, c(1.0)), np.where(scaled, gs, c(1.0))
        sf = (c(1.0) - angle / radius) * c(10.0)                                                  # :538
        e0, e1 = c(8.5), c(9.5) + (c(0.0) if brk == "smoothstep_no_haze" else haze / c(50.0))
        foot, top = dec.decide(sf <= e0, inside), dec.decide(sf >= e1, inside)
        dec.tag(inside & foot, "smoothstep 0"); dec.tag(inside & ~foot & ~top, "smoothstep rising"); dec.tag(inside & top, "smoothstep 1")
        sf = (np.power(sf / c(10.0), c(2.0 if brk == "glow_exponent_2" else 3.0)) * c(2.0) * glow_i * gs
              + fk.smoothstep(e0, e1, sf) * c(100.0) * disk_i * ds)                               # :540-541
        tint = np.where(col(inside), tint + sun_color * col(sf), tint)                            # :542
    out = tint * rgb_scale                                                                        # :546
    below = dec.decide(downness <= 0, live)                                                       # :547-579
    below = live & below
    dec.tag(below, "below the horizon: ground blend")
    irrad, path = calc_irrad(sun, c(2.0), c, brk)
    dec.path = path
    with np.errstate(all="ignore"):
        down = w[:, W_GROUND:W_GROUND + 3] * ((irrad + sun_color * col(sun[:, 2])) * rgb_scale)
        dim_g = dec.decide(factor < 1, below)
        down = np.where(col(dim_g), down * col(factor), down)
        blur = w[:, W_BLUR] / c(10.0)
        soft = dec.decide(blur > 0, below)
        dn = -downness / blur
        deep = dec.decide(dn > 1, below & soft)
        if brk != "dn_unclamped":
            dn = np.where(deep, c(1.0), dn)
        dec.tag(below & soft & deep, "dn > 1: clamped"); dec.tag(below & soft & ~deep & (dn > 0), "dn in (0, 1)"); dec.tag(below & ~soft, "horizon_blur <= 0")
        if brk == "dn_unclamped":
            dn = dn * dn * (c(3.0) - c(2.0) * dn)
        else:
            dn = fk.smoothstep(c(0.0), c(1.0), dn)
        blended = out * col(c(1.0) - dn) + down * col(dn)
    out = np.where(col(below), np.where(col(soft), blended, down), out)
    night_factor = np.where(below, np.where(soft, c(1.0) - dn, ft(0)), c(1.0))

    intensity = luminance(out, c)                                                                 # arch_colortweak :327-356
    grey = dec.decide(saturation <= 0, live)
    dec.tag(live & grey, "saturation <= 0: grey")
    out = np.where(col(grey), col(intensity), out * col(saturation) + col(intensity * (c(1.0) - saturation)))
    rbs = -w[:, W_RBS] if brk == "redblueshift_sign" else w[:, W_RBS]
    out = out * np.stack([c(1.0) + rbs, np.full(n, c(1.0)), c(1.0) - rbs], 1)
    dark = dec.decide(night_factor > 0, live)                                                     # :583-597
    night = w[:, W_NIGHT:W_NIGHT + 3] * col(night_factor)
    wins = out < night
    for k in range(3):
        dec.decide(wins[:, k], live & dark)
    dec.tag(live & dark & wins.any(1), "night colour wins a channel"); dec.tag(live & dark & ~wins.any(1), "night colour loses every channel")
    out = np.where(col(dark) & wins, night, out)
    out = out * PI                                                                                # :598
    with np.errstate(all="ignore"):
        ratio = np.where(enabled, angle / radius, np.inf)
    return np.where(col(zero), ft(0), out), dec, ratio, cos_sun


# ---- directions ----------------------------------------------------------------------------------------------------------------------------------------------
N_BAND, FAN = 120, (("core", 0.0, 0.044, 110), ("rise", 0.048, 0.148, 120), ("glow", 0.152, 0.94, 130), ("rim", 0.95, 1.05, 60), ("outside", 1.06, 2.5, 60))
N_FAN = sum(f[3] for f in FAN)


def untweak(r, words):
    """the input direction (float64) whose tweaked, untweaked-z direction (:311-324) is the unit vector r"""
    h = float(words[W_HH]) / 10.0
    lam = -h * r[:, 2] + np.sqrt(h * h * r[:, 2] ** 2 + 1.0 - h * h)
    o = r * lam[:, None]
    o[:, 2] += h
    return o[:, [0, 2, 1]] if np.ascontiguousarray(words).view(np.int32)[W_YUP] == 1 else o


def frame_of(s):
    a = np.array([0.0, 0.0, 1.0]) if abs(s[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    t = np.cross(s, a)
    t /= np.linalg.norm(t)
    return t, np.cross(s, t)


def extra_dirs(k, words):
    """band, fan and sun directions of settings row k -> ((n, 3) float32, nominal class per row)"""
    g = fk.Stream(max(N_BAND, N_FAN), 100 + k)
    sun = real_vectors(words[None], np.zeros((1, 3), np.float32), np.float64)[1][0]
    # band: tweaked z round 0 and round 0.001, down to -0.08 (dn > 1 needs z < -horizon_blur / 10) and up to 0.02
    z = np.concatenate([np.linspace(-0.08, -0.012, 30), np.linspace(-0.0098, -0.0002, 40), [0.0, -1e-6, 1e-6, 0.0005, 0.000999, 0.001001, float(np.float32(0.001)), 0.0015],
                        np.linspace(0.002, 0.02, N_BAND - 78)])
    phi = 2 * np.pi * g.u()[:N_BAND]
    rr = np.sqrt(1 - z * z)
    band = untweak(np.stack([rr * np.cos(phi), rr * np.sin(phi), z], 1), words).astype(np.float32)
    if words[W_HH] == 0:   # no normalize on the way in: the tweaked z IS the input word, so the thresholds themselves are hit exactly
        band[:, 1 if np.ascontiguousarray(words).view(np.int32)[W_YUP] == 1 else 2] = z.astype(np.float32)
    # fan: angle / sun_radius stratified per class; the radius of the defaults where the disc is off
    radius = float(np.float32(0.00465)) * float(words[W_DISK_S]) * 10.0 if words[W_DISK_S] > 0 else 0.2325
    t, b = frame_of(sun)
    ratio = np.concatenate([lo + (min(hi, 3.0 / radius) - lo) * (np.arange(m) + 0.5) / m for _, lo, hi, m in FAN])
    if not (words[W_DISK_S] > 0 and words[W_DISK_I] > 0):   # no disc: every fan row is of class outside, whose spread the sky alone cannot hold within
        ratio = 0.5 + 2.0 * (np.arange(N_FAN) + 0.5) / N_FAN   # half a nominal radius of the sun (acos near 1 again, in sky_luminance's gamma)
    az = 2 * np.pi * g.u()[:N_FAN]
    ang = ratio * radius
    fan = untweak(np.cos(ang)[:, None] * sun + np.sin(ang)[:, None] * (np.cos(az)[:, None] * t + np.sin(az)[:, None] * b), words).astype(np.float32)
    # the sun itself and its float32 neighbours
    s32 = untweak(sun[None], words).astype(np.float32)[0]
    near = [s32]
    for ax in range(3):
        for step in (-1, 1):
            v = s32.copy()
            v[ax] = np.nextafter(v[ax], np.float32(np.inf * step))
            near.append(v)
    near += [fk.f32_unit(s32[None].astype(np.float64))[0], np.float32(words[W_SUN:W_SUN + 3])]
    return np.concatenate([band, fan, np.array(near, np.float32)]), np.array([C_HORIZON] * N_BAND + [-1] * N_FAN + [C_SUN] * len(near))


def all_rows():
    """-> (words (S, 24), rows (n, 27), settings index per row, nominal class per row (-1: a fan row, classed by the model), extra directions per settings row)"""
    words = settings_words()
    sphere = fk.sky_dirs()
    rows, sidx, cls, extras = [], [], [], []
    for k in range(len(SETTINGS)):
        sp = sphere
        ex, ec = extra_dirs(k, words[k])
        d = np.concatenate([sp, ex])
        rows.append(np.concatenate([np.broadcast_to(words[k], (len(d), 24)), d], 1))
        sidx += [k] * len(d)
        cls += [C_SPHERE] * len(sp) + list(ec)
        extras.append(ex)
    return words, np.ascontiguousarray(np.concatenate(rows), np.float32), np.array(sidx, np.int16), np.array(cls, np.int8), np.array(extras, np.float32)


# ---- minting ---------------------------------------------------------------------------------------------------------------------------------------------------
def measure(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        num, den = np.abs(got - want).max(1), np.abs(want).max(1)
        e = np.where((num == 0) & (den == 0), 0.0, num / den)
    return np.where(np.isfinite(got).all(1) & np.isfinite(want).all(1), e, np.nan)


def iw_phys(w):
    return np.ascontiguousarray(w).view(np.int32)[:, W_PHYS]


def mint(brk=None):
    words, rows, sidx, cls, extras = all_rows()
    w, d = rows[:, :24], rows[:, 24:27]
    want, d64, ratio, cos64 = sun_and_sky(w, d, np.float64, brk)
    got32, d32, _, cos32 = sun_and_sky(w, d, np.float32, brk)
    assert len(d64.list) == len(d32.list)
    same = np.ones(len(rows), bool)
    for a, b in zip(d64.list, d32.list):
        same &= a == b
    same &= d64.path == d32.path
    # the fan rows are classed by the model's float64 evaluation
    inside = (d64.bits & BIT["inside the sun radius"]) != 0
    top, rising = (d64.bits & BIT["smoothstep 1"]) != 0, (d64.bits & BIT["smoothstep rising"]) != 0
    physical = (d64.bits & BIT["physically scaled"]) != 0
    fan = cls < 0
    rim = (ratio >= 0.95) & (ratio <= 1.05)
    lost = ((d64.bits & (BIT["inside the sun radius"] | BIT["outside the sun radius"])) != 0) & np.isnan(ratio)   # float64 dot above 1: the ray at the sun, never kept
    by_model = np.where(lost, np.where(iw_phys(w) == 1, C_CORE_PHYS, C_CORE), np.where(rim, C_RIM, np.where(~inside, C_OUTSIDE, np.where(top, np.where(physical, C_CORE_PHYS, C_CORE), np.where(rising, C_RISE, C_GLOW)))))
    cls = np.where(fan, by_model, cls).astype(np.int8)
    err = measure(got32, want)
    moved = np.zeros(len(rows))
    for nudge in (-DOT_NUDGE, DOT_NUDGE):
        m = measure(sun_and_sky(w, d, np.float64, brk, nudge)[0], want)
        moved = np.maximum(moved, np.where(np.isnan(m), np.inf, m))
    spread = np.array([SPREADS[c] for c in CLASSES])[cls]
    with np.errstate(invalid="ignore"):
        at_sun = (cos32 > 1) | (cos64 > 1 - DOT_MARGIN)
        kept = same & np.isfinite(err) & (err <= spread) & (moved <= spread) & ~at_sun
    out = dict(settings=words, setting_names=np.array([nm for nm, _ in SETTINGS]), extra_dirs=extras, sphere=fk.sky_dirs(), row_setting=sidx, row_class=cls, want=want, kept=kept, branches=d64.bits, branch_names=np.array(BRANCHES),
               class_names=np.array(CLASSES), class_spread=np.array([SPREADS[c] for c in CLASSES]), measure=np.array(MEASURE), SPREAD=np.float64(fk.SPREAD),
               at_sun=at_sun)
    return out, rows, err


def check_caps(out, report=False):
    """the caps of the kept mask -> (per class: rows, kept; per branch: kept rows); asserts them"""
    cls, kept, bits = out["row_class"], out["kept"], out["branches"]
    names = [str(c) for c in out["class_names"]]
    per_class = {c: (int((cls == k).sum()), int((kept & (cls == k)).sum())) for k, c in enumerate(names)}
    per_branch = {str(b): int((kept & ((bits >> np.uint64(k)) & np.uint64(1)).astype(bool)).sum()) for k, b in enumerate(out["branch_names"])}
    phys = out["settings"].view(np.int32)[out["row_setting"], W_PHYS]
    if report:
        print("class: rows / kept  " + ", ".join(f"{c} {a} / {b}" for c, (a, b) in per_class.items()))
        print("kept rows per branch: " + ", ".join(f"{b} {v}" for b, v in per_branch.items()))
    for c in DROP_CAPPED:
        a, b = per_class[c]
        assert a - b <= 0.02 * a, f"class {c}: {a - b} of {a} rows dropped (cap 2 %)"
    assert int((kept & (cls == C_CORE) & (phys == 0)).sum()) >= 50 and per_class["core"][1] >= 50, per_class["core"]
    assert per_class["core, physically scaled"][1] >= 50, per_class["core, physically scaled"]
    assert per_class["rise"][1] >= 30, per_class["rise"]
    short = {b: v for b, v in per_branch.items() if v < 50}
    assert not short, f"branches with fewer than 50 kept rows: {short}"
    return per_class, per_branch


def main(path=None, brk=None, caps=True):
    assert brk is None or brk in BREAK
    out, rows, err = mint(brk)
    if caps:
        for k, c in enumerate(CLASSES):
            m = out["row_class"] == k
            e = err[m & np.isfinite(err)]
            print(f"{c:24s} rows {int(m.sum()):6d} kept {int((m & out['kept']).sum()):6d}  float32 against float64: median {np.median(e):.2e} 99 % {np.percentile(e, 99):.2e} max {e.max():.2e}")
        check_caps(out, report=True)
    path = path or os.path.join(HERE, "sky_kat.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(rows), "rows of", len(SETTINGS), "settings")


if __name__ == "__main__":
    main()

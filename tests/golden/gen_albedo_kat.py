"""The float64 model of the demodulated history and the inputs its tests share.

Section 5.6 is sections 5.3 / 5.4 / 5.5 applied to another input and one product at the end, so the model RUNS the models of gen_temporal_kat.py and
gen_svgf_kat.py (imported, not copied) on the demodulated colour and multiplies at the end; nothing here restates them.

Definition
  a(g) = max(g, 0.001) per channel;  d(p) = c(p) / a(g_0(p)) per channel, a channel that is not finite passes through, alpha untouched
  step        section 5.3 (5.5: with the motion table) with d in the place of c: step 4's finiteness test is of d -- a finite c whose quotient exceeds
              FLT_MAX counts as not finite -- the blend is of d, and the moments (section 5.4) are of L(d) and L(d)^2.  The history's taps are read as stored.
  consumers   x(p) * a(g_0(p)) per channel for the final image x (after the last iteration, or Hc itself), a channel that is not finite passes through.

The bound.  `judge_step` hands the temporal model the quotient in float64, so that the reference is the definition in real numbers; the fp32 step reads
the quotient rounded once, at most u |d| away (u = 2^-24; a denormal step below the normal range).  The result is linear in the current colour with
coefficient a_blend = 1 / Hn' for BLEND, 1 for CURRENT and 0 otherwise, so 5.3's running first-order bound grows by a_blend (u |d| + denormal): ONE MORE u FOR THE
DIVISION AT THE INPUT.  (CURRENT pixels are also exact: the stored colour is the fp32 quotient bit for bit.)  The moments model takes the fp32 quotient
as its input, as gen_svgf_kat.moments takes every colour, and adds the error of L and L L itself; against the real quotient L moves by at most u |L|_1 and
L L by twice that relatively, through the same coefficient.  `remodulated` multiplies a judged image by a(g_0): an error e of the image becomes a e, and the
product adds u |x a| and a denormal step: ONE MORE u FOR THE PRODUCT AT THE OUTPUT.  The kept mask is the temporal model's own: its decisions are geometric
but for the finiteness of d, and the inputs keep that one clear of its edge (the planted quotients lie three orders of magnitude beyond FLT_MAX, every other
one thirty-odd below it), so the drop rates of section 5.3 carry over (cap 5 %).

Inputs: the sequences of gen_svgf_kat.py (the scene and moves of section 5.3: four static calls, then the move) and the cases of gen_motion_kat.py (section
5.5) at 96 x 64 and 45 x 37, with guide plane 0 replaced by `albedo_texture` -- one level per texel, uniform in [0.25, 1], with the values 0, -1, 0.001 and
0.0005 planted, never NaN -- and the colour 3e38 planted over albedo 0.001, the quotient that overflows.  The colours already hold NaN and +-Inf channels.

Run:  python tests/golden/measure_albedo_kat.py        (writes albedo_kat_tol.json; needs the host build of tests/albedo_host.py)
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "albedo_kat_tol.json")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sk = _load("gen_svgf_kat")
mk = _load("gen_motion_kat")
dk = _load("gen_denoise_kat")
tk = sk.tk
U, DENORMAL, FLT_MAX = tk.U, tk.DENORMAL, tk.FLT_MAX
SIZES, MOVES, MOTION_MOVES = tk.SIZES, tk.MOVES, mk.MOVES
FLOOR = 0.001   # PT_DENOISE_ALBEDO_FLOOR
DROP_CAP = 0.05
PLANTED = (0.0, -1.0, 0.001, 0.0005)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------
def albedo_texture(w, h, seed):
    """guide plane 0: one level per texel and channel, uniform in [0.25, 1]; alpha 1; PLANTED at seeded texels (all three channels, and single channels)"""
    rng = np.random.default_rng(9100 + seed)
    a = np.ones((h, w, 4), np.float32)
    a[..., :3] = rng.uniform(0.25, 1.0, (h, w, 3))
    for v in PLANTED:
        for _ in range(3 if w * h > 8 else 0):
            y, x = int(rng.integers(h)), int(rng.integers(w))
            a[y, x, :3] = v
            a[int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(3))] = v
    return a


def plant_overflow(colour, albedo, seed):
    """3e38 in a channel of a few pixels whose albedo is set to 0.001 there: finite, but the quotient is not"""
    h, w = colour.shape[:2]
    rng = np.random.default_rng(9200 + seed)
    spots = []
    for _ in range(4 if w * h > 8 else 0):
        y, x, j = int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(3))
        colour[y, x, :3] = np.where(np.isfinite(colour[y, x, :3]), colour[y, x, :3], 1.0)
        colour[y, x, j], albedo[y, x, j] = (-1.0 if len(spots) % 2 else 1.0) * 3.0e38, 0.001
        spots.append((y, x))
    return spots


def call_inputs(size, move, k):
    """gen_svgf_kat.call_inputs with the albedo texture as g0 and the overflowing quotients planted; inp["overflow"]: where"""
    inp = sk.call_inputs(size, move, k)
    seed = 100 * size[0] + 10 * k + (MOVES.index(move) if k >= sk.STATIC_CALLS else 0)
    inp["g0"] = albedo_texture(size[0], size[1], seed)
    inp["overflow"] = plant_overflow(inp["colour"], inp["g0"], seed)
    return inp


def motion_inputs(size, move):
    """gen_motion_kat.case_inputs with the albedo texture as g0 and the overflowing quotients planted (the fixture's history is read as it is: the
    history's taps are already demodulated)"""
    inp = mk.case_inputs(size, move)
    seed = 100 * size[0] + 7 * MOTION_MOVES.index(move) + 5
    inp["g0"] = albedo_texture(size[0], size[1], seed)
    inp["overflow"] = plant_overflow(inp["colour"], inp["g0"], seed)
    return inp


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------------------
def demodulate64(colour, albedo):
    """d in float64, (h, w, 4): the real quotient of the fp32 words; beyond FLT_MAX it is not finite for the step (+-Inf here)"""
    c = np.asarray(colour, np.float32).astype(np.float64)
    a = np.maximum(np.asarray(albedo, np.float32)[..., :3].astype(np.float64), np.float64(np.float32(FLOOR)))
    d = c.copy()
    with np.errstate(all="ignore"):
        q = c[..., :3] / a
        q = np.where(np.abs(q) > FLT_MAX, np.copysign(np.inf, q), q)
    d[..., :3] = np.where(np.isfinite(c[..., :3]), q, c[..., :3])
    return d


def judge_step(inp, judge=None):
    """The step of section 5.6 for one call: gen_temporal_kat.judge (or gen_motion_kat.judge for a case of motion_inputs) on the demodulated colour, with
    out_e grown by the division's u.  Returns the judged dict and d (float64)"""
    d = demodulate64(inp["colour"], inp["g0"])
    r = (judge or tk.judge)(dict(inp, colour=d))
    n = inp["w"] * inp["h"]
    a = np.where(r["outcome"] == tk.BLEND, 1.0 / np.maximum(r["length"], 1.0), np.where(r["outcome"] == tk.CURRENT, 1.0, 0.0))
    dd = np.where(np.isfinite(d[..., :3]), np.abs(d[..., :3]), 0.0).reshape(n, 3)
    r["out_e"] = r["out_e"] + a[:, None] * (U * dd + DENORMAL)
    return r, d


def judge_moments(inp, hm):
    """Hm' of the call: gen_svgf_kat.moments on the fp32 quotient (its input as it takes every colour), the bound grown by what the division's u does to L and
    L L through the blend factor.  Returns (m (n, 2), bound (n, 2), the temporal run)"""
    d32 = dk.demodulate(inp["colour"], inp["g0"])
    m, m_e, r = sk.moments(dict(inp, colour=d32), hm, np.float64)
    n = inp["w"] * inp["h"]
    fin = tk.finite3(d32.reshape(n, 4))
    c = np.where(fin[:, None], np.abs(d32.reshape(n, 4)[:, :3].astype(np.float64)), 0.0)
    l1 = 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]          # |L| <= l1, and |dL| <= u l1
    a = np.where(r["outcome"] == tk.BLEND, 1.0 / np.maximum(r["length"], 1.0), np.where(r["outcome"] == tk.CURRENT, 1.0, 0.0))
    grow = a[:, None] * np.stack([U * l1 + DENORMAL, 2.0 * U * l1 * l1 * (1.0 + U) + DENORMAL], 1)
    return m, m_e + np.where((r["outcome"] == tk.NOTHING)[:, None], 0.0, grow), r


def remodulated(x, x_e, albedo):
    """x (n, 3) float64 with bound x_e, times a(g_0): (value, bound); a value that is not finite passes through with bound 0"""
    a = np.maximum(np.asarray(albedo, np.float32).reshape(-1, 4)[:, :3].astype(np.float64), np.float64(np.float32(FLOOR)))
    with np.errstate(all="ignore"):
        fin = np.isfinite(x)
        v = np.where(fin, x * a, x)
        e = np.where(fin, a * x_e + U * np.abs(v) + DENORMAL, 0.0)
    return v, e

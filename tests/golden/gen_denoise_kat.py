"""Mints the DENOISER known answers in tests/golden/denoise_kat.npz and holds the float64 model they are judged by.

The model is written from the definition of the edge-avoiding a-trous filter (Dammertz et al. 2010) as DESIGN.md "Denoiser" states it, not from
vk_raytrace_amd/csrc/pt_denoise.h: numpy only, importing nothing of vk_raytrace_amd/, oracle/ or the other tests.

Definition (one iteration i, step s = 2^i, on a W x H RGBA32F image c with up to three guide planes g_j whose .xyz count)
  taps       q = p + s (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner; a tap outside the image is skipped; k = h[dx + 2] h[dy + 2], h = 1/16 1/4 3/8 1/4 1/16
  finite     a colour is finite when r, g and b are; a tap whose colour is not finite has weight 0 (it takes no part in either sum)
  exponent   e = dc inv_c(i) + d_0 inv_0 + d_1 inv_1 + d_2 inv_2, terms that are off left out; d_j = |g_j(p) - g_j(q)|^2 over xyz, dc the same over the
             colours of the iteration's input, left out when the colour term is off or the centre colour is not finite
  constants  fp32 BY DEFINITION: inv_c(i) = 1 / (s_i s_i), s_i = sigmaColor 2^-i; inv_j = 1 / (sigmaGuide_j sigmaGuide_j) -- `constants` below evaluates them in
             np.float32, every operation rounded once, which is what IEEE arithmetic gives anywhere
  weight     w = k exp(-e)
  output     rgb = sum(w c_q) / sum(w); sum(w) == 0: the centre unchanged; alpha = the centre's
  modulation with the flag: c.rgb / max(g_0.rgb, 0.001) before iteration 0 and c.rgb * max(g_0.rgb, 0.001) after the last; ONE IEEE operation per channel, so
             np.float32 reproduces it bit for bit (`demodulate`, `remodulate`); a channel that is not finite stays what it is under both

`iteration` evaluates one iteration in float64 on fp32 inputs and returns, next to the expectation, the bound the fp32 evaluation must meet; the derivation
of that bound is in the docstring of tests/test_denoise_model.py, next to the test that applies it, and `BOUND` below holds its constants.

Pixels the model does not judge (`left_out`): centre colour not finite AND 0 < sum(w) < 1e-30 in float64 -- there the underflow of the fp32 exp decides between a
mean and the unchanged pixel.  A float64 sum of exactly 0 is judged: the pixel must come back unchanged (e > 745 for every tap, far beyond where fp32 gives up).
Cap, asserted here on the model's own chain and again by the test on what it is fed: at most 1 % of a case's pixels per iteration.

Inputs: 70 x 45 and 33 x 64 images (and a 1 x 1), colour log-uniform in 1e-3 .. 1e3 with NaN, +Inf, -Inf and partly non-finite pixels inside regions where all
guides are flat (plus two next to an edge, one isolated by a depth spike and one nearly isolated), an albedo plane with a step edge and a patch below the floor, a normal plane with a ramp and a flat part, a depth
plane with a step of 1.0 and a ramp.  Cases: every on / off combination of the colour term, each guide and the demodulation (which needs guide 0), for 1, 5 and 8
iterations, so that the steps exceed the image.

Run:  python tests/golden/gen_denoise_kat.py            (rewrites denoise_kat.npz; deterministic)
      python tests/golden/gen_denoise_kat.py --measure  (then: writes denoise_kat_tol.json -- the bound's constants and the worst observed ratio of the host
                                                         build's error to the bound; needs the host build of tests/denoise_host.py)
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "denoise_kat.npz")
TOL_PATH = os.path.join(HERE, "denoise_kat_tol.json")

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
FLOOR = np.float32(0.001)
DEMODULATE = 1
SIZES = ((70, 45), (33, 64))            # (width, height)
ITERATIONS = (1, 5, 8)
SIGMA_COLOR = 2.0
SIGMA_GUIDE = (0.1, 0.25, 0.5)
LEFT_OUT_BELOW = 1e-30
LEFT_OUT_CAP = 0.01

# constants of the bound (tests/test_denoise_model.py derives them)
U = 2.0 ** -24
BOUND = {
    "u": U,
    "exponent_roundings": 8,         # per-tap exponent: 4 per distance (difference, square, two additions), 1 for the product with inv, 3 additions of 4 terms
    "exp_ulp": 1.1,                  # what tests/test_fpmath.py holds pt_exp to; 1 ulp <= 2 u relative in the normal range
    "exp_abs": 2.0 * 2.0 ** -149,    # ... and absolutely where the result is denormal or flushed (arguments below about -87.3)
    "denormal": 2.0 ** -149,         # absolute error of one fp32 operation whose result is denormal
    "taps": 25,                      # products per sum; a term passes through at most 24 additions
    "model_slack": 2.0 ** -20,       # relative allowance for the float64 evaluation's own rounding
}


def constants(sigma_color, sigma_guide):
    """inv_c[8], inv_g[3] in np.float32, each operation rounded once"""
    sc = np.float32(sigma_color)
    inv_c = np.zeros(8, np.float32)
    for i in range(8):
        s = np.float32(sc * np.float32(2.0 ** -i))
        inv_c[i] = np.float32(1.0) / np.float32(s * s) if sc > 0 else 0
    sg = np.asarray(sigma_guide, np.float32)
    return inv_c, np.float32(1.0) / (sg * sg).astype(np.float32)


def finite3(c):
    return np.isfinite(c[..., :3]).all(-1)


def _modulate(c, albedo, op):
    a = np.maximum(albedo[..., :3].astype(np.float32), FLOOR)
    out = c.astype(np.float32).copy()
    rgb = out[..., :3]
    fin = np.isfinite(rgb)
    with np.errstate(all="ignore"):
        rgb[fin] = op(rgb, a)[fin]
    return out


def demodulate(c, albedo):
    return _modulate(c, albedo, lambda x, a: (x / a).astype(np.float32))


def remodulate(c, albedo):
    return _modulate(c, albedo, lambda x, a: (x * a).astype(np.float32))


def _tap(a, oy, ox):
    """a shifted so that out[y, x] = a[y + oy, x + ox]; (out, inside) with out = 0 where the tap leaves the image"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def iteration(c32, guides, i, inv_c, inv_g, colour_term):
    """One iteration in float64.  c32: (H, W, 4) float32, the iteration's input; guides: three planes or None each; inv_c: the fp32 constant of THIS iteration
    (ignored without colour_term); inv_g: the three fp32 guide constants.  Returns a dict: `rgb` the expectation (H, W, 3), `bound` its absolute error bound per
    channel, `unchanged` pixels whose sum of weights is exactly 0 (expectation: the input's bits), `left_out` pixels the model does not judge, `sumw`."""
    B = BOUND
    u = B["u"]
    c = c32.astype(np.float64)
    h, w = c.shape[:2]
    step = 1 << i
    fin_p = finite3(c32)
    g64 = [None if g is None else g[..., :3].astype(np.float64) for g in guides]
    max_inv = max([float(inv_c) if colour_term else 0.0] + [float(inv_g[j]) for j in range(3) if g64[j] is not None] + [0.0])
    num, den = np.zeros((h, w, 3)), np.zeros((h, w))
    d_num, d_den = np.zeros((h, w, 3)), np.zeros((h, w))       # error bounds of the two fp32 sums
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = H5[dx + 2] * H5[dy + 2]
                cq, inside = _tap(c, step * dy, step * dx)
                fin_q, _ = _tap(fin_p, step * dy, step * dx)
                live = inside & fin_q
                cq3 = np.where(live[..., None], cq[..., :3], 0.0)
                e = np.zeros((h, w))
                if colour_term:
                    dc = ((np.where(fin_p[..., None], c[..., :3], 0.0) - cq3) ** 2).sum(-1)
                    e = e + np.where(fin_p, dc * float(inv_c), 0.0)
                for j in range(3):
                    if g64[j] is not None:
                        gq, _ = _tap(g64[j], step * dy, step * dx)
                        e = e + ((g64[j] - gq) ** 2).sum(-1) * float(inv_g[j])
                e = np.where(live, e, 0.0)
                wq = np.where(live, k * np.exp(-e), 0.0)
                # fp32 weight = wq (1 + delta) + eta: exponent off by at most 8 roundings (relative) and 8 denormal operations (absolute, scaled by the largest
                # constant); exp within exp_ulp ulp or exp_abs; one rounding for the product with k
                rho = np.expm1(np.minimum(e * ((1 + u) ** B["exponent_roundings"] - 1) + B["exponent_roundings"] * B["denormal"] * max_inv, 700.0))
                delta = (1 + rho) * (1 + B["exp_ulp"] * 2 * u) * (1 + u) - 1
                delta = np.where(wq > 0, delta, 0.0)           # (exp(-e) == 0 in float64: e > 745, the fp32 weight is 0 as well)
                eta = np.where(live, k * B["exp_abs"] + B["denormal"], 0.0)
                grow_n, grow_d = (1 + u) ** B["taps"], (1 + u) ** (B["taps"] - 1)
                num += wq[..., None] * cq3
                den += wq
                d_num += np.abs(wq[..., None] * cq3) * ((1 + delta[..., None]) * grow_n - 1) + (eta[..., None] * np.abs(cq3) + np.where(live, B["denormal"], 0.0)[..., None]) * grow_n
                d_den += wq * ((1 + delta) * grow_d - 1) + eta * grow_d
        unchanged = den == 0.0
        left_out = ~fin_p & (den > 0.0) & (den < LEFT_OUT_BELOW)
        judged = ~unchanged & ~left_out
        safe = np.where(judged, den, 1.0)
        rgb = np.where(judged[..., None], num / safe[..., None], c[..., :3])
        room = np.where(judged, den - d_den, 1.0)
        assert (room[judged] > 0.5 * den[judged]).all(), "the sum of weights of a judged pixel is not resolved in fp32"
        bound = (d_num + np.abs(rgb) * d_den[..., None]) / room[..., None] * (1 + u) + u * np.abs(rgb) + B["denormal"]
        bound = np.where(judged[..., None], bound * (1 + B["model_slack"]) + np.abs(rgb) * B["model_slack"] * u, 0.0)
    return {"rgb": rgb, "bound": bound, "unchanged": unchanged, "left_out": left_out, "sumw": den}


def chain(colour, guides, iterations, sigma_color, sigma_guide, flags):
    """The model alone through a whole call, each iteration's float64 result rounded to fp32 for the next (what the generator checks its cap on).  Yields
    (i, input of iteration i, result dict)."""
    inv_c, inv_g = constants(sigma_color, sigma_guide)
    cur = demodulate(colour, guides[0]) if flags & DEMODULATE else colour.astype(np.float32)
    for i in range(iterations):
        r = iteration(cur, guides, i, inv_c[i], inv_g, sigma_color > 0)
        yield i, cur, r
        nxt = cur.copy()
        keep = r["unchanged"] | r["left_out"]
        nxt[..., :3] = np.where(keep[..., None], cur[..., :3], r["rgb"].astype(np.float32))
        cur = nxt


def cases():
    """(colour term, (guide 0, 1, 2 installed), flags) for every valid combination"""
    out = []
    for col, g0, g1, g2, dem in itertools.product((0, 1), repeat=5):
        if dem and not g0:
            continue
        out.append((bool(col), (bool(g0), bool(g1), bool(g2)), DEMODULATE if dem else 0))
    return out


def case_guides(guides, installed):
    return [g if on else None for g, on in zip(guides, installed)]


def make_inputs(width, height, rng):
    """colour and the three guide planes of one size; the non-finite pixels sit in the block where every guide is flat, two more next to the albedo edge"""
    ys, xs = np.mgrid[0:height, 0:width]
    colour = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (height, width, 4))).astype(np.float32)
    colour[..., 3] = rng.uniform(0, 1, (height, width)).astype(np.float32)
    xe, ye = width // 2, height // 2
    albedo = np.zeros((height, width, 4), np.float32)
    albedo[..., :3] = np.where((xs < xe)[..., None], (0.8, 0.6, 0.4), (0.2, 0.3, 0.9))
    albedo[2:5, width - 6:width - 2, :3] = (0.0, 0.0005, 0.002)          # below and around the floor
    normal = np.zeros((height, width, 4), np.float32)
    ramp = (xs / max(width - 1, 1)).astype(np.float32)
    normal[..., 0] = np.where(ys < ye, ramp, 0.0)                        # a ramp above, flat below
    normal[..., 2] = np.where(ys < ye, np.sqrt(np.maximum(0.0, 1.0 - ramp.astype(np.float64) ** 2)), 1.0)
    depth = np.zeros((height, width, 4), np.float32)
    depth[..., 0] = np.where(ys < ye, 3.0 + 2.0 * ys / height, 6.0)       # a ramp above (below 4.0), a step of more than 1.0 at ye, flat below
    # flat in every guide: rows >= ye on either side of xe, away from it
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    flat = [(ye + 6, 5, (nan, nan, nan)), (ye + 8, 9, (inf, 1.0, 1.0)), (ye + 11, 4, (1.0, -inf, 2.0)), (ye + 7, width - 6, (0.5, 0.25, nan)),
            (ye + 12, width - 9, (inf, -inf, nan)), (ye + 13, width - 9, (nan, 1.0, 1.0)), (ye + 13, width - 8, (inf, inf, inf))]
    edge = [(ye + 9, xe - 1, (nan, 2.0, 2.0)), (ye - 1, 7, (inf, 3.0, 3.0))]
    for y, x, v in flat + edge:
        colour[min(y, height - 1), x, :3] = v
    # with the depth plane installed: a NaN pixel whose depth is 50 off its surroundings (e = 1e4, no tap has a weight: it comes back unchanged) and an Inf
    # pixel 6 off (e = 144, sum(w) ~ 1e-63: fp32 underflow decides, the one pixel the model leaves out); without the plane both are repaired
    colour[ye + 3, xe + 5, :3] = nan
    depth[ye + 3, xe + 5, 0] = 56.0
    colour[ye + 4, xe - 6, :3] = inf
    depth[ye + 4, xe - 6, 0] = 12.0
    return colour, [albedo, normal, depth]


def build():
    rng = np.random.default_rng(20101)
    out = {"sigma_color": np.float64(SIGMA_COLOR), "sigma_guide": np.array(SIGMA_GUIDE, np.float64), "iterations": np.array(ITERATIONS)}
    for w, h in SIZES:
        colour, guides = make_inputs(w, h, rng)
        out[f"colour_{w}x{h}"] = colour
        for name, g in zip(("albedo", "normal", "depth"), guides):
            out[f"{name}_{w}x{h}"] = g
    out["colour_1x1"] = np.array([[[0.25, 4.0, 100.0, 0.5]]], np.float32)
    for name in ("albedo", "normal", "depth"):
        out[f"{name}_1x1"] = np.array([[[0.5, 0.25, 0.125, 0.0]]], np.float32)
    return out


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def inputs(kat, w, h):
    return kat[f"colour_{w}x{h}"], [kat[f"{n}_{w}x{h}"] for n in ("albedo", "normal", "depth")]


def check_cap(kat):
    """the model alone stays within the left-out cap on every case and iteration"""
    worst = 0.0
    for w, h in SIZES:
        colour, guides = inputs(kat, w, h)
        for col, installed, flags in cases():
            for i, _, r in chain(colour, case_guides(guides, installed), max(ITERATIONS), SIGMA_COLOR if col else 0.0, SIGMA_GUIDE, flags):
                frac = r["left_out"].mean()
                worst = max(worst, frac)
                assert frac <= LEFT_OUT_CAP, f"{w}x{h} colour={col} guides={installed} flags={flags} iteration {i}: {frac:.4f} of the pixels left out"
    return worst


def measure():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import test_denoise_model as t
    worst = t.worst_ratio_over_fixture()
    rec = {"bound": BOUND, "left_out_below": LEFT_OUT_BELOW, "left_out_cap": LEFT_OUT_CAP,
           "measure": "max over judged pixels, channels, iterations and cases of |host fp32 - float64 model| / bound", "worst_ratio": worst}
    with open(TOL_PATH, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"worst ratio of the host build's error to the derived bound: {worst:.4f}")


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure()
    else:
        kat = build()
        print(f"largest left-out fraction of the model's own chains: {check_cap(kat):.4f}")
        np.savez_compressed(PATH, **kat)
        print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")

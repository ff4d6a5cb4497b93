"""Mints the SVGF known answers in tests/golden/svgf_kat.npz and holds the float64 model they are judged by.

The model is written from the definition of the variance-guided filter as DESIGN.md section 5.4 states it, not from vk_raytrace_amd/csrc/pt_svgf.h:
numpy, and the temporal model and scene of gen_temporal_kat.py (section 5.3), of which section 5.4 is an extension.

Definition
  L(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z;  usable(c) = c.rgb finite and L(c) finite;  san(v) = v > 0 ? min(v, FLT_MAX) : 0, on every READ of a variance
  moments    Hm' of a call: the colour step of section 5.3 applied to the planes (m1, m2) with the current value (Lc, Lc Lc) -- the same taps, weights, sw, outcome
             and blend factor: BLEND mix(h, (Lc, Lc Lc), a); HISTORY_ONLY h; CURRENT (Lc, Lc Lc); NOTHING (0, 0).  `moments` below therefore RUNS the temporal model
             on those planes: the history colour replaced by (m1, m2, 0), the current colour by (Lc, Lc Lc, 0), non-finite where the colours are, so that every
             verdict and the outcome are the colour step's.  Lc enters in the arithmetic of the run; its own error is added afterwards (the result is linear in it
             with coefficient a, or 1 for CURRENT).
  V0         n = Hn(p) >= minTemporal: v = m2 - m1 m1.  Otherwise over the 7 x 7 taps q (dy outer, dx inner) inside the image with Hn(q) >= 1 and Hc(q) finite:
             w = exp(-e), e the sum of the guide terms |g_j(p) - g_j(q)|^2 / sigma_j^2 of the installed planes in order (w = 1 without any);
             v = (s2 / sw - (s1 / sw)^2) (minTemporal / max(n, 1)) when sw > 0, else 0.  V0 = san(v)
  iteration  step s = 2^i.  vbar = sum g g san(V(q)) / sum g g over the 3 x 3 taps at step 1 inside the image, g = (1/4, 1/2, 1/4);  den = sigmaLum sqrt(vbar) + lumFloor.
             Over the 5 x 5 taps q = p + s (dx, dy) (dy outer, dx inner) inside the image with usable C(q): k = h(dx) h(dy), h = (1/16, 1/4, 3/8, 1/4, 1/16);
             e = |Lp - Lq| / den when the centre is usable, then the guide terms; w = k exp(-e) (w = k without any term); sums sr, sg, sb, sw of w C(q), w and
             sq of (w w) san(V(q)).  sw != 0: out = s / sw, Vout = sq / (sw sw); else out = C(p), Vout = san(V(p)).  Alpha is the centre's.

`iteration` / `variance0` run the definition in float64 or, the same statements, in float32 on fp32 inputs.  The float64 run carries gen_temporal_kat.V's running
first-order bound of what an fp32 evaluation of the same operations may differ by (u = 2^-24 per operation and one denormal step); exp adds 2.2 u of its value
(pt_exp is good to 1.1 ulp, an ulp is at most 2 u of the value) on top of exp(e) (e^{de} - 1) from its argument's own bound, which is the amplification by |e|: the
argument is good to about u |e|.  The square root takes the difference of the roots of the interval's ends, which at v = 0 is sqrt(dv) and away from it dv / (2 sqrt(v)):
max(., 0) and sqrt at 0 are continuous, so no pixel is dropped there, and lumFloor > 0 bounds what the root's error does to e.

Kept pixels.  The inputs of V0 and of an iteration are the host build's own previous outputs, which both runs share exactly: Hn(q) >= 1, the finiteness of the history's
colours and the usable test at iteration 0 compare inputs and need no margin.  Decisions that need one: n >= minTemporal (margin 1e-5; the fixtures use minTemporal =
3.5, between the integers a static camera gives), the usable test of colours that an earlier iteration computed (both runs must agree on every pixel a tap reads), and
sw > 0 / sw != 0 against a sum of vanishing weights (a sum below 1e-4 that is not empty drops the pixel).  The moments take the temporal model's own kept mask.
Cap (`check_caps`): at most 5 % of a case's pixels are dropped.

Inputs: the analytic scene and the moves of gen_temporal_kat.py at 96 x 64 and 45 x 37; the colour is a smooth function of the guides (so that regions have means of
their own) with seeded per-frame noise of 25 % of it added (so that no region has zero variance) and about 0.7 % non-finite channels.  A case is a sequence: four calls at
the start camera (lengths 1, 2, 3, 4: every pixel on the spatial branch up to the third, on the temporal one after the fourth), then the move.  The npz holds, for
45 x 37, the model's self-fed answers: the float32 run's histories as inputs, the float64 run's moments, V0 and five iterations for the yaw sequence.

Run:  python tests/golden/gen_svgf_kat.py            (rewrites svgf_kat.npz; deterministic)
      python tests/golden/measure_svgf_kat.py        (then: writes svgf_kat_tol.json; needs the host build of tests/svgf_host.py)
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "svgf_kat.npz")
TOL_PATH = os.path.join(HERE, "svgf_kat_tol.json")
_spec = importlib.util.spec_from_file_location("gen_temporal_kat", os.path.join(HERE, "gen_temporal_kat.py"))
tk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tk)

V, U, DENORMAL, FLT_MAX, MARGIN, SW_FLOOR = tk.V, tk.U, tk.DENORMAL, tk.FLT_MAX, tk.MARGIN, tk.SW_FLOOR
SIZES, STORED, MOVES = tk.SIZES, tk.STORED, tk.MOVES
DROP_CAP = 0.05
STATIC_CALLS = 4
MIN_TEMPORAL, SIGMA_LUM, LUM_FLOOR, SIGMA_GUIDE, ITERATIONS = 3.5, 4.0, 1e-4, (0.5, 0.3, 0.5), 5
NOISE = 0.25


def f32(x):
    """the fp32 constant, as a Python float: what both runs read"""
    return float(np.float32(x))


def params(iterations=ITERATIONS, sigma_lum=SIGMA_LUM, lum_floor=LUM_FLOOR, sigma_guide=SIGMA_GUIDE, min_temporal=MIN_TEMPORAL):
    return {"iterations": iterations, "sigmaLum": np.float32(sigma_lum), "lumFloor": np.float32(lum_floor), "sigmaGuide": np.asarray(sigma_guide, np.float32),
            "minTemporal": np.float32(min_temporal)}


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------
def scene_colour(g1, g2, rng, bad=0.007):
    """a smooth function of the guides, plus seeded noise of NOISE of it, about `bad` of the channels not finite; alpha 1"""
    h, w = g1.shape[:2]
    base = (0.3 + 1.5 * g1[..., :3].astype(np.float64)) * (4.0 / (4.0 + g2[..., :1].astype(np.float64)))
    c = np.ones((h, w, 4), np.float32)
    c[..., :3] = np.maximum(base * (1.0 + NOISE * rng.standard_normal((h, w, 3))), 0.0)
    hit = rng.uniform(size=(h, w, 3)) < bad
    c[..., :3][hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(hit.sum()))
    return c


def albedo_plane(g1, g2):
    """guide plane 0 of the scene: a step pattern per surface, exact in fp32"""
    a = np.ones(g1.shape, np.float32)
    a[..., :3] = np.round(g1[..., :3] * 4) / 4
    return a


def call_inputs(size, move, k):
    """what call k of the sequence of `move` reads besides the history: calls 0 .. STATIC_CALLS - 1 at the start camera, call STATIC_CALLS after the move"""
    w, h = size
    cam = tk.moved(move if k >= STATIC_CALLS else "none", w / h)
    g1, g2 = tk.guides(cam, w, h)
    rng = np.random.default_rng(77000 + 1000 * w + 10 * k + (MOVES.index(move) if k >= STATIC_CALLS else 0))
    return {"w": w, "h": h, "colour": scene_colour(g1, g2, rng), "g1": g1, "g2": g2, "g0": albedo_plane(g1, g2), "viewInverse": cam["viewInverse"],
            "projInverse": cam["projInverse"], "worldToClip": cam["worldToClip"], "depthTol": np.float32(tk.DEPTH_TOL), "normalDist2": np.float32(tk.NORMAL_DIST2),
            "maxHistory": np.float32(tk.MAX_HISTORY), "hist": None, "eye": cam["eye"], "center": cam["center"]}


def calls_of(move):
    return 1 if move == "first" else STATIC_CALLS + 1


# ---- pieces of the model --------------------------------------------------------------------------------------------------------------------------------------
def exact(x, ft):
    return V.exact(np.asarray(x, np.float32), ft, ft is np.float64)


def take(x, at):
    return V(x.v[at], None if x.e is None else x.e[at])


def vabs(x):
    return V(np.abs(x.v), x.e)


def vneg(x):
    return V(-x.v, x.e)


def vexp(x):
    z = np.exp(x.v)
    if x.e is None:
        return V(z)
    return V(z, z * np.expm1(np.minimum(x.e, 700.0)) + 2.2 * U * z + DENORMAL)


def san(x):
    with np.errstate(invalid="ignore"):
        return V(np.where(x.v > 0, np.minimum(x.v, x.v.dtype.type(FLT_MAX)), x.v.dtype.type(0)), x.e)


def lum(c):
    return (c[0] * f32(0.2126) + c[1] * f32(0.7152)) + c[2] * f32(0.0722)


def tap(h, w, dx, dy):
    """flat index of (x + dx, y + dy) for every pixel (0 where outside) and whether it lies inside the image"""
    ys, xs = np.mgrid[0:h, 0:w]
    qx, qy = xs + dx, ys + dy
    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    return np.where(inside, qy * w + qx, 0).reshape(-1), inside.reshape(-1)


def b3(i):
    return (0.0625, 0.25, 0.375, 0.25, 0.0625)[i + 2]


def guide_terms(guides, prm, ft):
    """[(plane as three V, 1 / sigma^2 as the fp32 word)] of the installed planes, in order"""
    out = []
    for j, g in enumerate(guides or (None, None, None)):
        if g is None:
            continue
        s = np.float32(prm["sigmaGuide"][j])
        out.append(([exact(g.reshape(-1, 4)[:, k], ft) for k in range(3)], float(np.float32(1.0) / (s * s))))
    return out


def guide_chain(e, terms, at):
    """e + t_0 + t_1 + ... in plane order (e None: the chain starts with t_0); None when there is no term at all"""
    for plane, inv in terms:
        d = [plane[k] - take(plane[k], at) for k in range(3)]
        t = tk.dot3(d, d) * inv
        e = t if e is None else e + t
    return e


# ---- moments -------------------------------------------------------------------------------------------------------------------------------------------------
def moments(inp, hm, ft):
    """Hm' of one call in arithmetic `ft`: (m (n, 2), bound (n, 2) or None).  inp as gen_temporal_kat.case_inputs gives it (hist None: a first call), hm (h, w, 2)"""
    w, h = inp["w"], inp["h"]
    n = w * h
    c = inp["colour"].reshape(n, 4)
    fin = tk.finite3(c)
    C = [exact(np.where(fin, c[:, j], 0), ft) for j in range(3)]
    with np.errstate(all="ignore"):
        L = lum(C)
        L2 = L * L
    assert (np.abs(L2.v) < 1e30).all()
    sub = np.zeros((n, 4), ft)
    sub[:, 0], sub[:, 1] = L.v, L2.v
    sub[~fin, :3] = np.nan
    sub_inp = dict(inp, colour=sub.reshape(h, w, 4))
    if inp["hist"] is not None:
        hc = np.zeros((n, 4), np.float32)
        hc[:, :2] = np.asarray(hm, np.float32).reshape(n, 2)
        hc[~tk.finite3(inp["hist"]["colour"].reshape(n, 4)), :3] = np.nan
        sub_inp["hist"] = dict(inp["hist"], colour=hc.reshape(h, w, 4))
    r = tk.evaluate(sub_inp, ft)
    nothing = r["outcome"] == tk.NOTHING
    m = np.where(nothing[:, None], 0, r["out"][:, :2])
    if ft is not np.float64:
        return m, None, r
    a = np.where(r["outcome"] == tk.BLEND, 1.0 / np.maximum(r["length"], 1.0), np.where(r["outcome"] == tk.CURRENT, 1.0, 0.0))
    e = r["out_e"][:, :2] + a[:, None] * np.stack([L.e, L2.e], 1)
    return m, np.where(nothing[:, None], 0.0, e), r


# ---- V0 ------------------------------------------------------------------------------------------------------------------------------------------------------
def variance0(hist_colour, hist_length, hist_moments, guides, prm, ft):
    """V0 in arithmetic `ft`: dict of v, v_e (float64 only), ok, temporal (the branch taken)"""
    h, w = hist_length.shape
    n = h * w
    fin = tk.finite3(hist_colour.reshape(n, 4))
    hn = hist_length.reshape(n)
    m1, m2 = exact(hist_moments.reshape(n, 2)[:, 0], ft), exact(hist_moments.reshape(n, 2)[:, 1], ft)
    N, mt = exact(hn, ft), f32(prm["minTemporal"])
    terms = guide_terms(guides, prm, ft)
    with np.errstate(all="ignore"):
        temporal = hn >= np.float32(mt)
        ok = np.abs(hn.astype(np.float64) - mt) >= MARGIN * np.maximum(np.abs(hn), mt)
        vt = m2 - m1 * m1
        zero = exact(np.zeros(n), ft)
        s1, s2, sw = zero, zero, zero
        some = np.zeros(n, bool)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                at, inside = tap(h, w, dx, dy)
                act = inside & (hn[at] >= 1) & fin[at]
                e = guide_chain(None, terms, at)
                wt = exact(np.ones(n), ft) if e is None else vexp(vneg(e))
                s1 = (s1 + wt * take(m1, at)).where(act, s1)
                s2 = (s2 + wt * take(m2, at)).where(act, s2)
                sw = (sw + wt).where(act, sw)
                some |= act
        have = sw.v > 0
        ok &= temporal | ~some | (sw.v >= SW_FLOOR)
        safe = sw.where(have, 1.0)
        mean = s1 / safe
        boost = exact(np.float32(mt), ft) / N.where(hn >= 1, 1.0)
        vs = ((s2 / safe - mean * mean) * boost).where(have, 0.0)
        v = san(vt.where(temporal, vs))
    return {"v": v.v, "v_e": v.e, "ok": ok, "temporal": temporal, "have": have}


def judge_variance0(hist_colour, hist_length, hist_moments, guides, prm):
    r64, r32 = (variance0(hist_colour, hist_length, hist_moments, guides, prm, ft) for ft in (np.float64, np.float32))
    r64["kept"] = r64["ok"] & r32["ok"] & (r64["have"] == r32["have"])
    return r64


# ---- one iteration -------------------------------------------------------------------------------------------------------------------------------------------
def iteration(colour, var, guides, prm, i, ft):
    """iteration i in arithmetic `ft` over the image: dict of out (n, 3), var, their bounds out_e, var_e (float64 only), ok, usable, nz (sw != 0)"""
    h, w = var.shape
    n = h * w
    s = 1 << i
    c = colour.reshape(n, 4)
    fin = tk.finite3(c)
    with np.errstate(all="ignore"):
        C = [exact(np.where(fin, c[:, j], 0), ft) for j in range(3)]
        L = lum(C)
        usable = fin & (np.abs(L.v) <= FLT_MAX)
        Vs = san(exact(var.reshape(n), ft))
        zero = exact(np.zeros(n), ft)
        sv, sgs = zero, zero
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                at, inside = tap(h, w, dx, dy)
                g = (0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)
                sv = (sv + take(Vs, at) * g).where(inside, sv)
                sgs = (sgs + g).where(inside, sgs)
        den = (sv / sgs).sqrt() * f32(prm["sigmaLum"]) + f32(prm["lumFloor"])
        terms = guide_terms(guides, prm, ft)
        sums = [zero] * 5
        some = np.zeros(n, bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                at, inside = tap(h, w, s * dx, s * dy)
                act = inside & usable[at]
                kk = b3(dx) * b3(dy)
                e_on = guide_chain(vabs(L - take(L, at)) / den, terms, at)
                e_off = guide_chain(None, terms, at)
                w_on = vexp(vneg(e_on)) * kk
                w_off = exact(np.full(n, kk), ft) if e_off is None else vexp(vneg(e_off)) * kk
                wt = w_on.where(usable, w_off)
                vals = [take(C[j], at) for j in range(3)]
                adds = [wt * vals[0], wt * vals[1], wt * vals[2], wt, (wt * wt) * take(Vs, at)]
                sums = [(sums[j] + adds[j]).where(act, sums[j]) for j in range(5)]
                some |= act
        sr, sg, sb, sw, sq = sums
        nz = sw.v != 0
        ok = ~some | (sw.v >= SW_FLOOR)
        safe = sw.where(nz, 1.0)
        out = [(x / safe).where(nz, 0.0) for x in (sr, sg, sb)]
        vout = (sq / (safe * safe)).where(nz, Vs)
    res = {"out": np.stack([np.where(nz, out[j].v, c[:, j].astype(ft)) for j in range(3)], 1), "var": vout.v, "ok": ok, "usable": usable, "nz": nz}
    if ft is np.float64:
        res["out_e"], res["var_e"] = np.stack([o.e for o in out], 1), vout.e
    return res


def judge_iteration(colour, var, guides, prm, i):
    """the float64 run with its bounds, and `kept`: both runs decide alike with their margins, on the pixel and on every pixel a tap of it reads"""
    r64, r32 = (iteration(colour, var, guides, prm, i, ft) for ft in (np.float64, np.float32))
    kept = r64["ok"] & r32["ok"] & (r64["nz"] == r32["nz"])
    differs = r64["usable"] != r32["usable"]
    if differs.any():
        h, w = var.shape
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                at, inside = tap(h, w, (1 << i) * dx, (1 << i) * dy)
                kept &= ~(inside & differs[at])
    r64["kept"], r64["run32"] = kept, r32
    return r64


def check_caps(kept_by_name, report=False):
    for name, kept in kept_by_name.items():
        dropped = 1 - kept.mean()
        if report:
            print(f"{name:40s} dropped {100 * dropped:5.2f} %")
        if dropped > DROP_CAP:
            raise AssertionError(f"{name}: {100 * dropped:.2f} % of the pixels are dropped (cap {100 * DROP_CAP} %)")


# ---- the model feeding itself (the fixture; the tests feed it the host build's outputs instead) ------------------------------------------------------------------
def self_fed(size, move, iterations=ITERATIONS):
    """The sequence of `move` with the float32 run's outputs as each call's history.  Returns per call a dict: inp, temporal (judged colour step), m, m_e, hm (the
    float32 moments that become history), and for the last call v0 (judged) and steps (judged iterations, each fed the float32 run of the one before)."""
    w, h = size
    hist, hm, calls = None, None, []
    for k in range(calls_of(move)):
        inp = call_inputs(size, "first" if move == "first" else move, k)
        inp["hist"] = hist
        judged = tk.judge(inp)
        m64, m_e, _ = moments(inp, hm, np.float64)
        m32, _, _ = moments(inp, hm, np.float32)
        r32 = judged["run32"]
        colour = inp["colour"].copy()
        colour[..., :3] = r32["out"].reshape(h, w, 3)
        guide = inp["g1"].copy()
        guide[..., 3] = inp["g2"][..., 0]
        hist = {"colour": colour, "guide": guide, "length": r32["length"].reshape(h, w).astype(np.float32), "worldToClip": inp["worldToClip"],
                "eye": inp["viewInverse"][12:15].copy()}
        hm = m32.reshape(h, w, 2).astype(np.float32)
        calls.append({"inp": inp, "temporal": judged, "m": m64, "m_e": m_e, "hm": hm, "hist": hist})
    last = calls[-1]
    prm = params(iterations)
    guides = (last["inp"]["g0"], last["inp"]["g1"], last["inp"]["g2"])
    last["v0"] = judge_variance0(hist["colour"], hist["length"], hm, guides, prm)
    c = hist["colour"]
    v = variance0(hist["colour"], hist["length"], hm, guides, prm, np.float32)["v"].reshape(h, w).astype(np.float32)
    last["steps"] = []
    for i in range(iterations):
        r = judge_iteration(c, v, guides, prm, i)
        last["steps"].append(r)
        nxt = c.copy()
        nxt[..., :3] = r["run32"]["out"].reshape(h, w, 3)
        c, v = nxt, r["run32"]["var"].reshape(h, w).astype(np.float32)
    return calls


def main():
    kept = {}
    for size in SIZES:
        for move in MOVES:
            calls = self_fed(size, move)
            name = f"{size[0]}x{size[1]} {move}"
            for k, call in enumerate(calls):
                kept[f"{name} call {k} moments"] = call["temporal"]["kept"]
            kept[f"{name} V0"] = calls[-1]["v0"]["kept"]
            for i, r in enumerate(calls[-1]["steps"]):
                kept[f"{name} iteration {i}"] = r["kept"]
            if size == STORED and move == "yaw":
                stored = calls
    check_caps(kept, report=True)
    last = stored[-1]
    out = {"m": last["m"], "m_e": np.minimum(last["m_e"], 1e38).astype(np.float32), "m_kept": last["temporal"]["kept"], "V0": last["v0"]["v"],
           "V0_e": np.minimum(last["v0"]["v_e"], 1e38).astype(np.float32), "V0_kept": last["v0"]["kept"]}
    for i, r in enumerate(last["steps"]):
        out[f"c{i}"], out[f"c{i}_e"] = r["out"], np.minimum(r["out_e"].max(1), 1e38).astype(np.float32)
        out[f"v{i}"], out[f"v{i}_e"], out[f"k{i}"] = r["var"], np.minimum(r["var_e"], 1e38).astype(np.float32), r["kept"]
    np.savez_compressed(PATH, **out)
    print(f"{PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    sys.exit(main())

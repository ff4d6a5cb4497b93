"""The float64 model of the responsive history and the inputs its tests share.

Section 5.7 is two steps of sections 5.3 / 5.5 / 5.6 and one clamp.  The steps are the models of gen_temporal_kat.py, gen_motion_kat.py and gen_albedo_kat.py
(imported, not copied): `step_models` RUNS them twice, once as they stand and once with (Hf, Hnf) in the place of (Hc, Hn) and maxFast in the place of
maxHistory.  Only the clamp is stated here.

Definition of the clamp (R = radius, k = sigmaScale; in place on Hc', Hn'; Hf', Hnf' are what the fast step wrote)
  p is left untouched when !(Hn'(p) >= 1) or Hc'(p).rgb is not finite.
  taps q = p + (dx, dy), dy = -R .. R outer, dx = -R .. R inner; skipped when outside the image, when !(Hnf'(q) >= 1) or when Hf'(q).rgb is not finite.
  per channel, in tap order:  n += 1;  s1 += f;  s2 += f f.   n < 2: untouched.
  mu = s1 / n;  v = s2 / n - mu mu;  sigma = sqrt(v < 0 ? 0 : v) (a NaN passes through);  lo = mu - k sigma;  hi = mu + k sigma.   Any lo or hi not finite:
  untouched.
  x' = min(max(x, lo), hi) per channel; alpha untouched; if any x' != x: Hn'(p) = min(Hn'(p), maxFast).  Hm' untouched.

`clamp` runs these statements in float64 or, the same statements, in float32 on fp32 inputs -- the float32 run has to give the host build's bits, since
nothing but +, *, / and sqrt is involved.  The float64 run carries gen_temporal_kat.V's running first-order bound (u = 2^-24 per operation and one denormal
step): n is a count and exact; s1 and s2 grow by u |sum| per addition and u |f f| per product; mu by the quotient's rule; v = s2 / n - mu mu carries the
bound of both of its terms and u |v|, as V0 of section 5.4 does; the square root takes the difference of the roots of the interval's ends, so that it is
continuous at 0 as in section 5.4.  x' is continuous in lo and hi -- |x'_64 - x'_32| <= max(|dlo|, |dhi|) whichever side x lies on -- so x < lo and x > hi are
no decisions for the colour.  They are decisions for Hn' (margin 1e-5 of max(|x|, |bound|), and the bound's own error): `kept_n`.  v < 0 (against the
size of s2 / n) and the finiteness of lo and hi -- and of the sums they are made of, which in fp32 overflow on the way: f f beyond FLT_MAX makes hi
infinite by the definition's own arithmetic -- are decisions with the margin for both: `kept`.  The inputs of the clamp are the host build's own step
outputs, which both runs share exactly: Hn' >= 1, Hnf' >= 1 and the finiteness of stored colours compare inputs and need no margin.
Cap: at most 5 % of a case's pixels are dropped from the Hn' judgement.

Inputs: the sequences of gen_svgf_kat.py (four static calls, then the move; seeded noise of 25 % on every pixel, so that sigma > 0 wherever n >= 2) and the
cases of gen_motion_kat.py at 96 x 64 and 45 x 37, with gen_albedo_kat.py's texture where the history is demodulated.  FAST: maxFast = 2.5 (the fixture's
sequences have four static calls at maxHistory = 6: the two histories differ from the third call on; and between the integers a static camera gives, so
that the imported model's min(N + 1, maxFast) keeps its margin), sigmaScale = 1 (about a third of the pixels clamp, so that both branches of Hn' are well
filled), radius = 2.

Run:  python tests/golden/measure_fast_kat.py        (writes fast_kat_tol.json; needs the host build of tests/fast_host.py)
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "fast_kat_tol.json")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ak = _load("gen_albedo_kat")
sk, mk, dk, tk = ak.sk, ak.mk, ak.dk, ak.tk
V, U, DENORMAL, FLT_MAX, MARGIN = tk.V, tk.U, tk.DENORMAL, tk.FLT_MAX, tk.MARGIN
SIZES, MOVES, MOTION_MOVES = tk.SIZES, tk.MOVES, mk.MOVES
DROP_CAP = 0.05
FAST = {"maxFast": np.float32(2.5), "sigmaScale": np.float32(1.0), "radius": 2}


def fast_history_for(inp, seed):
    """a fast history for a fixture that has only a long one (gen_motion_kat's cases): another seeded colour, finite where the long one is, and the long
    length capped at FAST's maxFast"""
    H = inp["hist"]
    rng = np.random.default_rng(8800 + seed)
    hf = tk.noisy_colour(inp["w"], inp["h"], rng)
    hf[..., :3] = np.where(np.isfinite(H["colour"][..., :3]), np.where(np.isfinite(hf[..., :3]), hf[..., :3], 1.0), H["colour"][..., :3])
    return hf, np.minimum(H["length"], FAST["maxFast"]).astype(np.float32)


# ---- the two steps: the imported models ------------------------------------------------------------------------------------------------------------------------
def step_models(inp, fast_hist, prm, demodulated=False, judge=None):
    """(long, fast): the judged step of the section the settings select -- gen_temporal_kat.judge, `judge` (gen_motion_kat.judge for a moving case), or
    gen_albedo_kat.judge_step around either -- as it stands, and on (Hf, Hg, Hnf) with maxFast.  inp["hist"] None: a first call (fast_hist is not read).
    fast_hist: (Hf (h, w, 4), Hnf (h, w))"""
    fast_inp = dict(inp, maxHistory=np.float32(prm["maxFast"]))
    if inp["hist"] is not None:
        fast_inp["hist"] = dict(inp["hist"], colour=fast_hist[0], length=fast_hist[1])
    run = (lambda i: ak.judge_step(i, judge)[0]) if demodulated else (judge or tk.judge)
    return run(inp), run(fast_inp)


# ---- the clamp -------------------------------------------------------------------------------------------------------------------------------------------------
def clamp(hf, hnf, hc, hn, prm, ft):
    """The clamp in arithmetic `ft` over the image.  Returns a dict of flat arrays: out (n, 3), length, n, mu / sigma / lo / hi (n, 3; NaN where the pixel
    was left before they were formed), moved, touched (the pixel went through the clamp), the decisions ok (colour) and ok_n (Hn'), and -- float64
    only -- the bounds out_e, mu_e, sigma_e, lo_e, hi_e"""
    track = ft is np.float64
    h, w = np.asarray(hn).shape
    n = w * h
    R, k, mf = int(prm["radius"]), float(np.float32(prm["sigmaScale"])), np.float32(prm["maxFast"])
    f, c = np.asarray(hf, np.float32).reshape(n, 4), np.asarray(hc, np.float32).reshape(n, 4)
    nf, nl = np.asarray(hnf, np.float32).reshape(n), np.asarray(hn, np.float32).reshape(n)
    K = lambda x: V.exact(x, ft, track)   # noqa: E731
    with np.errstate(all="ignore"):
        counts = (nf >= 1) & tk.finite3(f)
        own = (nl >= 1) & tk.finite3(c)
        cnt = np.zeros(n, ft)
        s1, s2 = [K(np.zeros(n)) for _ in range(3)], [K(np.zeros(n)) for _ in range(3)]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                at, inside = sk.tap(h, w, dx, dy)
                act = inside & counts[at]
                cnt = cnt + np.where(act, 1, 0).astype(ft)
                for j in range(3):
                    fq = K(np.where(act, f[at, j], 0))
                    s1[j] = (s1[j] + fq).where(act, s1[j])
                    s2[j] = (s2[j] + fq * fq).where(act, s2[j])
        enough = own & (cnt >= 2)
        N = K(np.where(enough, cnt, 1))
        dec = tk.Decisions(n)
        alive = enough.copy()
        mu, sigma, lo, hi = [], [], [], []
        for j in range(3):
            m = s1[j] / N
            mean2 = s2[j] / N
            v = mean2 - m * m
            neg = v.v < 0
            dec.compare(enough, v.v, 0.0, neg, np.abs(mean2.v))
            sg = v.where(~neg, 0.0).sqrt()
            ks = sg * k
            l, u = m - ks, m + ks
            for q in (s1[j], s2[j], l, u):
                alive &= dec.finite(enough, q.v)
            mu.append(m), sigma.append(sg), lo.append(l), hi.append(u)
        x = c[:, :3].astype(ft)
        out = np.stack([np.where(alive, np.minimum(np.maximum(x[:, j], lo[j].v), hi[j].v), x[:, j]) for j in range(3)], 1)
        # the decisions of Hn': on which side of each bound the colour lies
        ok_n = np.ones(n, bool)
        for j in range(3):
            for b in (lo[j], hi[j]):
                gap = np.abs(x[:, j].astype(np.float64) - b.v.astype(np.float64))
                need = MARGIN * np.maximum(np.abs(x[:, j]), np.abs(b.v)).astype(np.float64) + (2.0 * b.e if track else 0.0)
                ok_n &= ~alive | (gap >= need)
        moved = alive & (out != x).any(1)
        length = np.where(moved, np.minimum(nl, mf), nl).astype(ft)
    nan3 = lambda parts: np.where(enough[:, None], np.stack([p.v for p in parts], 1), np.nan)   # noqa: E731
    res = {"out": out, "length": length, "n": np.where(own, cnt, 0), "mu": nan3(mu), "sigma": nan3(sigma), "lo": nan3(lo), "hi": nan3(hi), "moved": moved, "touched": alive,
           "enough": enough, "ok": dec.ok, "ok_n": dec.ok & ok_n, "log": np.stack(dec.log, 1)}
    if track:
        for name, parts in (("mu", mu), ("sigma", sigma), ("lo", lo), ("hi", hi)):
            res[name + "_e"] = np.stack([p.e for p in parts], 1)
        res["out_e"] = np.where(alive[:, None], np.maximum(res["lo_e"], res["hi_e"]), 0.0)
    return res


def judge_clamp(hf, hnf, hc, hn, prm):
    """the float64 run with its bounds; `kept`: the pixels whose decisions for the colour have their margin in both runs and agree; `kept_n`: ... for Hn'
    as well; `run32`: the float32 run"""
    r64, r32 = (clamp(hf, hnf, hc, hn, prm, ft) for ft in (np.float64, np.float32))
    same = (r64["log"] == r32["log"]).all(1) & (r64["touched"] == r32["touched"])
    r64["kept"] = r64["ok"] & r32["ok"] & same
    r64["kept_n"] = r64["kept"] & r64["ok_n"] & r32["ok_n"] & (r64["moved"] == r32["moved"])
    r64["run32"] = r32
    return r64


# ---- what it is for: a one-channel sketch of both routes in float64 ------------------------------------------------------------------------------------------
def response(frames, switch, max_history, prm, w=64, h=64, noise=0.25, before=1.0, after=3.0, seed=0, clamped=True):
    """A static camera on a flat surface in float64, one channel repeated: `switch` calls of illumination `before`, then `after`, each with seeded Gaussian
    noise of `noise` of it.  Returns per call (rmse against the clean image of that call, mean Hn')."""
    rng = np.random.default_rng(seed)
    R, k, mf = int(prm["radius"]), float(prm["sigmaScale"]), float(prm["maxFast"])
    hc = hf = hn = hnf = None
    out = []
    for t in range(frames):
        level = before if t < switch else after
        cur = level * (1.0 + noise * rng.standard_normal((h, w)))
        if hc is None:
            hc, hf, hn, hnf = cur.copy(), cur.copy(), np.ones((h, w)), np.ones((h, w))
        else:
            hn, hnf = np.minimum(hn + 1.0, max_history), np.minimum(hnf + 1.0, mf)
            hc, hf = hc * (1.0 - 1.0 / hn) + cur / hn, hf * (1.0 - 1.0 / hnf) + cur / hnf
        if clamped:
            pad = np.pad(hf, R, constant_values=np.nan)
            taps = np.stack([pad[R + dy:R + dy + h, R + dx:R + dx + w] for dy in range(-R, R + 1) for dx in range(-R, R + 1)])
            cnt = np.isfinite(taps).sum(0)
            mu = np.nansum(taps, 0) / cnt
            sg = np.sqrt(np.maximum(np.nansum(taps * taps, 0) / cnt - mu * mu, 0.0))
            new = np.minimum(np.maximum(hc, mu - k * sg), mu + k * sg)
            hn = np.where(new != hc, np.minimum(hn, mf), hn)
            hc = new
        out.append((float(np.sqrt(np.mean((hc - level) ** 2))), float(hn.mean())))
    return out

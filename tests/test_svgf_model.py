"""The variance-guided filter of the history: the host build of vk_raytrace_amd/csrc/pt_svgf.h (tests/svgf_host.py) against the
float64 model of the definition (tests/golden/gen_svgf_kat.py), its exact properties, what the estimate and the filter are for, and planted breaks.  No
GPU: tests/test_svgf_gpu.py holds the device to this host build bit for bit.

The bound is derived, not measured: the model's float64 run carries with every value a running first-order bound of an fp32 evaluation of the same
operation sequence (gen_temporal_kat.V; exp and the square root as gen_svgf_kat.py states them), applied as it stands with 2^-20 relative slack for the
float64 evaluation's own rounding.  Every stage is judged from the host build's own previous output -- the history of the call before, the colour and
variance of the iteration before -- so that errors do not compound.  tests/golden/measure_svgf_kat.py records the worst error over bound per output in
svgf_kat_tol.json: reported, not used.

Kept pixels: the model alone decides (gen_svgf_kat.py, "Kept pixels"); at most 5 % of a case may be dropped, which is asserted for every case.

Planted breaks (test_a_planted_break_fails_its_test applies each to a scratch copy of the header, never to the tree, and runs the named check):
    w not squared in sq                          exact_propagation
    the prefilter left out                       filter_meets_model (yaw)
    the prefilter taken at step s                filter_meets_model (yaw)
    sigmaLum multiplying vbar, not its root      filter_meets_model (yaw)
    the boost left out                           filter_meets_model (first: every pixel on the spatial branch)
    moments gathered over all four taps          moments_meet_model (yaw)
    m1 m1 - m2                                   filter_meets_model (none: every pixel on the temporal branch)
    san missing on the tap read                  hostile_variance
    tap order dx outer                           tap_order_is_exact
    the luminance term on for an unusable centre nan_repair
"""
import importlib.util
import os

import numpy as np
import pytest

from tests import svgf_host as sh, temporal_host as th
from vk_raytrace_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_svgf_kat", os.path.join(ROOT, "tests", "golden", "gen_svgf_kat.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
tk = gen.tk

SLACK = 1.0 + 2.0 ** -20
CASES = [(size, move) for size in gen.SIZES for move in gen.MOVES]
IDS = [f"{s[0]}x{s[1]}-{m}" for s, m in CASES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def temporal_params(inp):
    return th.params(inp["worldToClip"], float(inp["depthTol"]), float(inp["normalDist2"]), float(inp["maxHistory"]))


def svgf_params(prm):
    return sh.params(int(prm["iterations"]), float(prm["sigmaLum"]), float(prm["lumFloor"]), tuple(float(v) for v in prm["sigmaGuide"]), float(prm["minTemporal"]))


def hist_dict(hist):
    return None if hist is None else {"colour": hist.colour, "guide": hist.guide, "length": hist.length, "worldToClip": hist.world_to_clip, "eye": hist.eye}


_sequences = {}


def run_sequence(size, move, L=None):
    """the calls of a case on the host build, each fed the one before: [(inputs with that history, the history read or None, the history written)].  The
    four static calls are the same for every move and computed once."""
    out, hist = [], None
    for k in range(gen.calls_of(move)):
        key = (size, k if k < gen.STATIC_CALLS else move)
        if L is None and key in _sequences:
            out.append(_sequences[key])
        else:
            inp = gen.call_inputs(size, move, k)
            inp["hist"] = hist_dict(hist)
            rc, new = sh.temporal_m(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], temporal_params(inp), hist, L=L)
            assert rc == 0
            out.append((inp, hist, new))
            if L is None:
                _sequences[key] = out[-1]
        hist = out[-1][2]
    return out


def worst_ratio(err, bound, sel):
    with np.errstate(all="ignore"):
        r = np.where(sel, err / (bound * SLACK + 1e-300), 0.0)
    assert not np.isnan(r).any()
    return float(np.max(r, initial=0.0))


# ---- moments -------------------------------------------------------------------------------------------------------------------------------------------------
def check_moments(size, move, L=None):
    """every call of the sequence: Hm' within the model's bound on the temporal model's kept pixels; colour, guide and length bit-identical to a call without
    moments.  Returns the worst error over bound."""
    worst = 0.0
    n = size[0] * size[1]
    calls = run_sequence(size, move, L)
    for k, (inp, hist, new) in enumerate(calls if move in ("none", "first") else calls[-1:]):
        kept = tk.judge(inp)["kept"]
        assert 1 - kept.mean() <= gen.DROP_CAP, (size, move, k)
        m, m_e, r = gen.moments(inp, None if hist is None else hist.moments, np.float64)
        got = new.moments.reshape(n, 2).astype(np.float64)
        worst = max(worst, worst_ratio(np.abs(got - m), m_e, kept[:, None] & np.ones(2, bool)))
        exact = kept & (r["outcome"] == tk.NOTHING)
        assert (bits(new.moments.reshape(n, 2)[exact]) == 0).all()
        rc, plain = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], temporal_params(inp),
                                None if hist is None else th.History(hist.colour, hist.guide, hist.length, hist.world_to_clip, hist.eye))
        assert rc == 0
        for a, b in ((new.colour, plain.colour), (new.guide, plain.guide), (new.length, plain.length)):
            assert np.array_equal(bits(a), bits(b)), f"{size} {move} call {k}: tracking moments changed the history"
    assert worst <= 1.0, f"{size} {move}: moments error / bound {worst}"
    return worst


@pytest.mark.parametrize("size,move", CASES, ids=IDS)
def test_moments_meet_model(size, move):
    check_moments(size, move)


# ---- V0 and the iterations -----------------------------------------------------------------------------------------------------------------------------------
def guides_of(inp, which=(0, 1, 2)):
    return tuple(inp[f"g{j}"] if j in which else None for j in range(3))


def check_filter(size, move, L=None, which=(0, 1, 2), iterations=gen.ITERATIONS):
    """V0 of the history the sequence leaves, then every iteration, each judged from the host build's own input to it.  Returns {output: worst error / bound}"""
    w, h = size
    n = w * h
    inp, _, hist = run_sequence(size, move, L)[-1]
    guides, prm = guides_of(inp, which), gen.params(iterations)
    p = svgf_params(prm)
    worst = {}
    j = gen.judge_variance0(hist.colour, hist.length, hist.moments, guides, prm)
    rc, v0 = sh.variance(hist.colour, hist.length, hist.moments, guides, p, L=L)
    assert rc == 0 and 1 - j["kept"].mean() <= gen.DROP_CAP
    assert (v0 >= 0).all() and np.isfinite(v0).all()
    worst["v0"] = worst_ratio(np.abs(v0.reshape(n).astype(np.float64) - j["v"]), j["v_e"], j["kept"])
    if move == "none":
        assert j["temporal"].mean() > 0.9
    if move == "first":
        assert not j["temporal"].any()
    if move == "disocclude":
        assert 0.15 < j["temporal"].mean() < 0.85
    c, v = hist.colour, v0
    for i in range(iterations):
        r = gen.judge_iteration(c, v, guides, prm, i)
        rc, c2, v2 = sh.iteration(c, v, guides, p, i, L=L)
        assert rc == 0 and 1 - r["kept"].mean() <= gen.DROP_CAP
        judged = r["kept"] & r["nz"]
        worst[f"colour {i}"] = worst_ratio(np.abs(c2.reshape(n, 4)[:, :3].astype(np.float64) - r["out"]), r["out_e"], judged[:, None] & np.ones(3, bool))
        worst[f"variance {i}"] = worst_ratio(np.abs(v2.reshape(n).astype(np.float64) - r["var"]), r["var_e"], r["kept"])
        same = r["kept"] & ~r["nz"]          # nothing usable around: the centre unchanged
        assert np.array_equal(bits(c2.reshape(n, 4)[same]), bits(c.reshape(n, 4)[same]))
        assert np.array_equal(bits(c2[..., 3]), bits(c[..., 3]))
        c, v = c2, v2
    assert all(x <= 1.0 for x in worst.values()), f"{size} {move} guides {which}: error / bound {worst}"
    return worst


@pytest.mark.parametrize("size,move", CASES, ids=IDS)
def test_filter_meets_model(size, move):
    check_filter(size, move)


@pytest.mark.parametrize("which", [(), (1,), (0, 2)], ids=["no-guide", "normal-only", "albedo-depth"])
def test_filter_meets_model_with_fewer_planes(which):
    check_filter((45, 37), "disocclude", which=which, iterations=3)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_generator_mints_and_meets_its_caps():
    kat = np.load(gen.PATH)
    calls = gen.self_fed(gen.STORED, "yaw")
    last = calls[-1]
    kept = {f"call {k}": c["temporal"]["kept"] for k, c in enumerate(calls)}
    kept["V0"] = last["v0"]["kept"]
    assert np.array_equal(kat["m"], last["m"]) and np.array_equal(kat["m_kept"], last["temporal"]["kept"])
    assert np.array_equal(kat["V0"], last["v0"]["v"]) and np.array_equal(kat["V0_kept"], last["v0"]["kept"])
    for i, r in enumerate(last["steps"]):
        assert np.array_equal(kat[f"c{i}"], r["out"], equal_nan=True) and np.array_equal(kat[f"v{i}"], r["var"]) and np.array_equal(kat[f"k{i}"], r["kept"])
        kept[f"iteration {i}"] = r["kept"]
    gen.check_caps(kept)
    # the float32 run of the model lies within the float64 run's bound of it: the bound bounds what it says it does
    n = gen.STORED[0] * gen.STORED[1]
    for i, r in enumerate(last["steps"]):
        sel = r["kept"] & r["nz"]
        assert worst_ratio(np.abs(r["run32"]["out"].astype(np.float64) - r["out"]), r["out_e"], sel[:, None] & np.ones(3, bool)) <= 1.0
        assert worst_ratio(np.abs(r["run32"]["var"].astype(np.float64) - r["var"]), r["var_e"], r["kept"]) <= 1.0


# ---- exact properties ----------------------------------------------------------------------------------------------------------------------------------------
def check_exact_propagation(L=None):
    """constant colour, no guide, V a constant power of two: an interior pixel of iteration 0 gives V 4900 / 65536 bit for bit (sum h^2 = 70 / 256 per axis) and
    its colour unchanged bit for bit"""
    w, h = 23, 17
    c = np.empty((h, w, 4), np.float32)
    c[...] = (0.75, 0.3, 1.7, 0.5)
    for k in (-20, -3, 0, 7, 40):
        v = np.full((h, w), 2.0 ** k, np.float32)
        rc, c2, v2 = sh.iteration(c, v, None, sh.params(1), 0, L=L)
        assert rc == 0
        inner = (slice(2, h - 2), slice(2, w - 2))
        assert (bits(v2[inner]) == bits(np.float32(2.0 ** k * 4900 / 65536))).all()
        assert np.array_equal(bits(c2[inner]), bits(c[inner]))


def test_exact_propagation():
    check_exact_propagation()


def hostile_planes(rng, h, w):
    v = rng.uniform(0, 2, (h, w)).astype(np.float32)
    hit = rng.uniform(size=(h, w)) < 0.3
    v[hit] = rng.choice(np.array([np.nan, -1.0, -0.0, np.inf, 3e38, -np.inf], np.float32), int(hit.sum()))
    return v


def check_hostile_variance(L=None):
    """variance planes with NaN, -1, -0, +Inf, -Inf and 3e38: the output colour is finite wherever the input is, no NaN reaches a colour, and the variance that
    comes out is finite and not negative; the planes sanitised beforehand give the same bits"""
    rng = np.random.default_rng(11)
    w, h = 41, 29
    c = rng.uniform(0.1, 3.0, (h, w, 4)).astype(np.float32)
    for i in range(3):
        v = hostile_planes(rng, h, w)
        rc, c2, v2 = sh.iteration(c, v, None, sh.params(3), i, L=L)
        assert rc == 0 and np.isfinite(c2).all() and np.isfinite(v2).all() and (v2 >= 0).all()
        with np.errstate(invalid="ignore"):
            clean = np.where(v > 0, np.minimum(v, np.float32(gen.FLT_MAX)), np.float32(0)).astype(np.float32)
        rc, c3, v3 = sh.iteration(c, clean, None, sh.params(3), i, L=L)
        assert np.array_equal(bits(c2), bits(c3)) and np.array_equal(bits(v2), bits(v3))


def test_hostile_variance():
    check_hostile_variance()


def check_nan_repair(L=None):
    """section 5.1's repair and isolation here: a pixel that is not usable is rebuilt from its usable neighbours, and what it holds reaches no other pixel"""
    rng = np.random.default_rng(12)
    w, h = 37, 23
    inp = gen.call_inputs((w, h), "none", 0)
    guides = guides_of(inp)
    c = rng.uniform(0.1, 3.0, (h, w, 4)).astype(np.float32)
    v = rng.uniform(0, 0.5, (h, w)).astype(np.float32)
    hit = rng.uniform(size=(h, w)) < 0.05
    for g in (None, guides):
        outs = []
        for junk in ((np.nan, 1.0, 1.0), (np.inf, -np.inf, 5.0), (-np.inf, np.nan, 0.0)):
            c1 = c.copy()
            c1[hit, :3] = junk
            rc, c2, v2 = sh.iteration(c1, v, g, sh.params(2), 0, L=L)
            assert rc == 0 and np.isfinite(c2).all() and np.isfinite(v2).all()
            outs.append((c2, v2))
        for c2, v2 in outs[1:]:
            assert np.array_equal(bits(c2[..., :3]), bits(outs[0][0][..., :3])) and np.array_equal(bits(v2), bits(outs[0][1]))


def test_nan_repair_and_isolation():
    check_nan_repair()


def check_tap_order(L=None):
    """where no exponential is involved -- an unusable centre, no guide plane: w = k -- every operation is an IEEE one and the sums run in the stated order, so
    the model's float32 run gives the host build's bits"""
    rng = np.random.default_rng(13)
    w, h = 33, 21
    c = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 4))).astype(np.float32)
    v = rng.uniform(0, 2, (h, w)).astype(np.float32)
    hit = rng.uniform(size=(h, w)) < 0.2
    c[hit, 0] = np.nan
    prm = gen.params(2)
    differing = 0
    for i in (0, 1):
        r = gen.iteration(c, v, None, prm, i, np.float32)
        rc, c2, v2 = sh.iteration(c, v, None, svgf_params(prm), i, L=L)
        sel = hit.reshape(-1) & r["nz"]
        assert sel.sum() > 50
        assert np.array_equal(bits(c2.reshape(-1, 4)[sel, :3]), bits(r["out"][sel])) and np.array_equal(bits(v2.reshape(-1)[sel]), bits(r["var"][sel]))


def test_tap_order_is_exact():
    check_tap_order()


def test_svgf_constants_refuses_with_its_own_reason():
    assert sh.constants(sh.params(1)) == (0, "") and sh.constants(sh.params(8, 1e-30, 1e-30, (1.0, 1.0, 1.0), 1.0), 7) == (0, "")
    assert sh.constants(sh.params(3, sigma_guide=(np.nan, -1.0, 0.0)), 0) == (0, "")          # read for installed planes only
    cases = [(None, 0, "null")] + [(sh.params(i), 0, "iterations") for i in (0, 9, -1)]
    cases += [(sh.params(2, sigma_lum=x), 0, "sigmaLum") for x in (0.0, -1.0, np.nan, np.inf)]
    cases += [(sh.params(2, lum_floor=x), 0, "lumFloor") for x in (0.0, -1.0, np.nan, np.inf)]
    cases += [(sh.params(2, min_temporal=x), 0, "minTemporal") for x in (0.99, np.nan, np.inf)]
    cases += [(sh.params(2, sigma_guide=(1.0, x, 1.0)), 2, "positive and finite") for x in (0.0, -1.0, np.nan, np.inf)]
    cases += [(sh.params(2, sigma_guide=(1.0, 1.0, 1e-30)), 4, "overflows"), (sh.params(2, flags=1), 0, "flag"), (sh.params(2, flags=0x80000000), 0, "flag")]
    reasons = set()
    for p, planes, word in cases:
        rc, why = sh.constants(p, planes)
        assert rc == capi.PT_ERR_INVALID and word in why, (word, why)
        reasons.add(why)
    assert len(reasons) == 8


def test_pt_exp_of_a_large_negative_argument_is_zero():
    """what the weights rely on (tests/test_fpmath.py pins it on the device; this is the host build of the same header): an exponent that overflows, from a
    luminance difference over a tiny divisor, gives weight 0 and not NaN"""
    c = np.ones((5, 5, 4), np.float32)
    c[2, 2, :3] = 3e30
    rc, c2, v2 = sh.iteration(c, np.zeros((5, 5), np.float32), None, sh.params(1, lum_floor=1e-30), 0)
    assert rc == 0 and np.isfinite(c2).all()
    assert np.array_equal(bits(c2[2, 2]), bits(c[2, 2])) and (c2[0, 0, :3] == 1).all()          # the outlier keeps to itself: every weight across the step is 0


# ---- what it is for ------------------------------------------------------------------------------------------------------------------------------------------
def static_history(colours, max_history=64.0, L=None):
    """N calls with a static camera over the given colour images, constant guides (normal up, depth 5): the history they leave"""
    h, w = colours[0].shape[:2]
    cam = tk.moved("none", w / h)
    g1, g2 = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    g1[...] = (0.5, 1.0, 0.5, 1.0)
    g2[..., 0] = 5.0
    p = th.params(cam["worldToClip"], tk.DEPTH_TOL, tk.NORMAL_DIST2, max_history)
    hist = None
    for c in colours:
        rc, hist = sh.temporal_m(c, g1, g2, cam["viewInverse"], cam["projInverse"], p, hist, L=L)
        assert rc == 0
    return hist


def grey(lum, noise):
    c = np.ones(lum.shape + (4,), np.float32)
    c[..., :3] = (lum + noise)[..., None]
    return c


@pytest.mark.parametrize("calls", [8, 4])
def test_the_estimate_means_what_it_says(calls):
    """i.i.d. Gaussian noise of standard deviation sigma on a flat image, N calls of a static camera: the mean of V0 lies within 5 % of sigma^2 (N - 1) / N (the
    float64 prototype was 0.5 - 0.6 % off at N = 8 and 1.9 % at N = 4; the standard error of the mean is about 0.7 %)"""
    w, h, sigma = 96, 64, 0.1
    for seed in range(2):
        rng = np.random.default_rng(100 + seed)
        hist = static_history([grey(np.ones((h, w)), sigma * rng.standard_normal((h, w))) for _ in range(calls)])
        assert (hist.length == calls).all()
        rc, v0 = sh.variance(hist.colour, hist.length, hist.moments, None, sh.params(1, min_temporal=3.5))
        want = sigma * sigma * (calls - 1) / calls
        print(f"N = {calls} seed {seed}: mean V0 {v0.mean():.6f}, sigma^2 (N - 1) / N {want:.6f}, off by {100 * (v0.mean() / want - 1):+.2f} %")
        assert rc == 0 and abs(v0.mean() / want - 1) <= 0.05


def check_the_filter_stops_at_the_edge(L=None):
    """luminance 1 left and 4 right, sigma 0.5, N = 8, 5 iterations, sigmaLum 4, lumFloor 1e-4, no guide: the RMSE against the clean image is below 0.25 x the
    unfiltered history's, and below that of the same filter with the luminance term out of action (sigmaLum 1e30)"""
    w, h, sigma, calls = 96, 64, 0.5, 8
    clean = np.where(np.arange(w)[None, :] < w // 2, 1.0, 4.0) * np.ones((h, 1))
    worst = 0.0
    for seed in range(3):
        rng = np.random.default_rng(200 + seed)
        hist = static_history([grey(clean, sigma * rng.standard_normal((h, w))) for _ in range(calls)], L=L)

        def rmse(img):
            return float(np.sqrt(np.mean((img[..., 0].astype(np.float64) - clean) ** 2)))
        rc, _, steps = sh.filter_history(hist, None, sh.params(5, 4.0, 1e-4), L=L)
        rc2, _, blind = sh.filter_history(hist, None, sh.params(5, 1e30, 1e-4), L=L)
        assert rc == 0 and rc2 == 0
        e_hist, e_filter, e_blind = rmse(hist.colour), rmse(steps[-1][0]), rmse(blind[-1][0])
        print(f"seed {seed}: RMSE unfiltered {e_hist:.4f}, filtered {e_filter:.4f} ({e_filter / e_hist:.3f} of it), luminance term disabled {e_blind:.4f}")
        assert e_filter < 0.25 * e_hist and e_filter < e_blind
        worst = max(worst, e_filter / e_hist)
    return worst


def test_the_filter_does_what_it_is_for():
    check_the_filter_stops_at_the_edge()


# ---- planted breaks ------------------------------------------------------------------------------------------------------------------------------------------
TAP_LOOPS = """  for(int dy = -2; dy <= 2; ++dy)
  {
    const int qy = y + step * dy;
    if(qy < 0 || qy >= h)
      continue;
    for(int dx = -2; dx <= 2; ++dx)
    {
      const int qx = x + step * dx;
      if(qx < 0 || qx >= w)
        continue;
"""
TAP_LOOPS_DX_OUTER = """  for(int dx = -2; dx <= 2; ++dx)
  {
    const int qx = x + step * dx;
    if(qx < 0 || qx >= w)
      continue;
    for(int dy = -2; dy <= 2; ++dy)
    {
      const int qy = y + step * dy;
      if(qy < 0 || qy >= h)
        continue;
"""
BREAKS = {
    "w_not_squared": (("sq + (wt * wt) * sv_san", "sq + wt * sv_san"), lambda L: check_exact_propagation(L)),
    "no_prefilter": (("const float vbar = sv / sgs;", "const float vbar = sv_san(src.variance(x, y));"), lambda L: check_filter((45, 37), "yaw", L)),
    "prefilter_at_step": (("const int vy = y + dy;", "const int vy = y + step * dy;"), lambda L: check_filter((45, 37), "yaw", L)),
    "sigma_inside_root": (("k.sigmaLum * sqrtf(vbar)", "sqrtf(k.sigmaLum * vbar)"), lambda L: check_filter((45, 37), "yaw", L)),
    "no_boost": ((" * (k.minTemporal / (n >= 1.0f ? n : 1.0f));", ";"), lambda L: check_filter((45, 37), "first", L)),
    "all_four_taps": (("if(pr.verdict[i] == 1)", "if(pr.verdict[i] != 0 && pr.verdict[i] != 2)"), lambda L: check_moments((96, 64), "yaw", L)),
    "variance_negated": (("v           = m.y - m.x * m.x;", "v           = m.x * m.x - m.y;"), lambda L: check_filter((45, 37), "none", L)),
    "no_san_on_tap": (("(wt * wt) * sv_san(src.variance(qx, qy))", "(wt * wt) * src.variance(qx, qy)"), lambda L: check_hostile_variance(L)),
    "dx_outer": ((TAP_LOOPS, TAP_LOOPS_DX_OUTER), lambda L: check_tap_order(L)),
    "lum_term_for_unusable_centre": (("if(lumOn)", "if(true)"), lambda L: check_nan_repair(L)),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_a_planted_break_fails_its_test(name, tmp_path):
    (old, new), check = BREAKS[name]
    text = open(os.path.join(sh.CSRC, "pt_svgf.h")).read()
    assert text.count(old) == 1, name
    tmp = str(tmp_path)
    open(os.path.join(tmp, "pt_svgf.h"), "w").write(text.replace(old, new))
    L = sh.bind(sh.compile_to(os.path.join(tmp, "libbroken.so"), header_dir=tmp))
    with pytest.raises(AssertionError):
        check(L)

"""The demodulated history: the host build of vk_raytrace_amd/csrc/pt_albedo.h in front of pt_temporal.h, pt_motion.h and pt_svgf.h
(tests/albedo_host.py) against the existing host builds fed the divided colour, bit for bit; against the float64 model (tests/golden/gen_albedo_kat.py);
what the feature is for; its refusals; planted breaks.  No GPU: tests/test_albedo_gpu.py holds the device to this host build bit for bit, and the
context's state (the setting, the history's mark) to the definition.

Composition.  gen_denoise_kat.demodulate reproduces the division bit for bit in np.float32, so the adaptor in front of temporal_pixel / temporal_pixel_moving
/ svgf_moments has to give what the parent's host builds (temporal_host, svgf_host.temporal_m, motion_host.temporal_moving) give on the divided colour: on
every bit of colour, guide, length and moments, for all four combinations of (moments, moving).

The bound against the model is section 5.3's running first-order bound with one more u = 2^-24 for the division at the input and one for the product at the
output (gen_albedo_kat's docstring derives it), applied as it stands with the 2^-20 slack of tests/test_temporal_model.py.  measure_albedo_kat.py records
the worst ratio in albedo_kat_tol.json: reported, not used.

Planted breaks (test_a_planted_break_fails_its_test applies each to scratch copies of the headers or to the host build's unit, never to the tree):
    moments taken from the raw colour            composition (the moments differ from svgf_host's on the divided colour)
    remodulation by the history's position       what_it_is_for_checkerboard (the contrast of a one-pixel checkerboard collapses under a one-pixel shift)
    floor missing                                remodulation_is_the_denoisers (albedo 0, -1 and 0.0005 are planted)
    remodulating twice                           what_it_is_for_checkerboard (the contrast becomes 1.5625)
    demodulating the gathered taps               composition (a second static call no longer equals temporal_host on the divided colour)
"""
import importlib.util
import os
import tempfile

import numpy as np
import pytest

from tests import albedo_host as ah, motion_host as mh, svgf_host as sh, temporal_host as th
from tests import test_temporal_model as tmodel
from vk_raytrace_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_albedo_kat", os.path.join(ROOT, "tests", "golden", "gen_albedo_kat.py"))
ak = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ak)
sk, mk, dk, tk = ak.sk, ak.mk, ak.dk, ak.tk
bits, SLACK = tmodel.bits, tmodel.SLACK
SIZES = tk.SIZES
SEQ_CASES = [(size, move) for size in SIZES for move in tk.MOVES]
MOTION_CASES = [(size, move) for size in SIZES for move in mk.MOVES]
IDS = lambda cases: [f"{s[0]}x{s[1]}-{m}" for s, m in cases]   # noqa: E731


def params_of(inp):
    return th.params(inp["worldToClip"], float(inp["depthTol"]), float(inp["normalDist2"]), float(inp["maxHistory"]))


def same(a, b, moments):
    ok = np.array_equal(bits(a.colour), bits(b.colour)) and np.array_equal(bits(a.guide), bits(b.guide)) and np.array_equal(bits(a.length), bits(b.length))
    return ok and (not moments or np.array_equal(bits(a.moments), bits(b.moments)))


# ---- the sequences on the new host build ---------------------------------------------------------------------------------------------------------------------
_sequences = {}


def run_sequence(size, move, moments, L=None):
    """the calls of a case on the new host build, each fed the one before: [(inputs, the history read or None, the history written)]"""
    out, hist = [], None
    for k in range(sk.calls_of(move)):
        key = (size, k if k < sk.STATIC_CALLS else move, moments)
        if L is None and key in _sequences:
            out.append(_sequences[key])
        else:
            inp = ak.call_inputs(size, move, k)
            rc, new = ah.temporal(inp["colour"], inp["g0"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), hist, moments=moments, L=L)
            assert rc == 0
            out.append((inp, hist, new))
            if L is None:
                _sequences[key] = out[-1]
        hist = out[-1][2]
    return out


# ---- composition, bit for bit ---------------------------------------------------------------------------------------------------------------------------------
def check_composition_static(size, move, moments, L=None):
    """every call of the sequence: the adaptor on (colour, albedo) is the parent's host build on the divided colour"""
    for k, (inp, hist, new) in enumerate(run_sequence(size, move, moments, L)):
        d = dk.demodulate(inp["colour"], inp["g0"])
        assert d.dtype == np.float32
        if moments:
            old = None if hist is None else sh.History(hist.colour, hist.guide, hist.length, hist.moments, hist.world_to_clip, hist.eye)
            rc, want = sh.temporal_m(d, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), old)
        else:
            rc, want = th.temporal(d, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), hist)
        assert rc == 0 and same(new, want, moments), f"{size} {move} call {k} moments {moments}: not the parent's host build on the divided colour"
        # the pixels whose quotient overflows take the outcome of a colour that is not finite: no blend, and a first call stores length 0
        for (y, x) in inp["overflow"]:
            assert not np.isfinite(d[y, x, :3]).all() and np.isfinite(inp["colour"][y, x, :3]).all()
            if hist is None:
                assert new.length[y, x] == 0.0
            else:
                assert np.array_equal(bits(new.length[y, x]), bits(want.length[y, x])) and new.length[y, x] <= max(hist.length.max(), 1.0)


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size,move", SEQ_CASES, ids=IDS(SEQ_CASES))
def test_composition_static(size, move, moments):
    check_composition_static(size, move, moments)


def moving_history(inp, moments, rng):
    H = inp["hist"]
    hm = np.exp(rng.uniform(-3, 3, (inp["h"], inp["w"], 2))).astype(np.float32) if moments else None
    return mh.History(H["colour"], H["guide"], H["length"], H["worldToClip"], H["eye"], hm)


def run_moving(inp, moments, hist, L=None):
    tab = None if hist is None else mh.table(inp["hist_words"], inp["cur_words"])
    rc, new, outcome = ah.temporal(inp["colour"], inp["g0"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), hist, moments=moments,
                                   ids=inp["ids"], tab=tab, want_outcome=True, L=L)
    assert rc == 0
    return new, outcome, tab


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size,move", MOTION_CASES, ids=IDS(MOTION_CASES))
def test_composition_moving(size, move, moments):
    """the moving form: a first call, then the move on the fixture's history"""
    inp = ak.motion_inputs(size, move)
    d = dk.demodulate(inp["colour"], inp["g0"])
    for hist in (None, moving_history(inp, moments, np.random.default_rng(5))):
        new, _, tab = run_moving(inp, moments, hist)
        rc, want = mh.temporal_moving(d, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), inp["ids"], tab, hist, moments=moments)
        assert rc == 0 and same(new, want, moments), f"{size} {move} moments {moments} history {hist is not None}"
        for (y, x) in inp["overflow"]:
            assert not np.isfinite(d[y, x, :3]).all()
            assert new.length[y, x] == 0.0 if hist is None else np.array_equal(bits(new.length[y, x]), bits(want.length[y, x]))


def check_remodulation_is_the_denoisers(L=None):
    """x * max(g, floor) per channel as gen_denoise_kat.remodulate states it, over the texture with its planted 0, -1, 0.001 and 0.0005 and over colours with
    NaN, +-Inf (which pass through, payload and all) and values whose product is denormal"""
    rng = np.random.default_rng(21)
    for (w, h) in SIZES:
        g = ak.albedo_texture(w, h, 3)
        x = sk.scene_colour(*tk.guides(tk.moved("none", w / h), w, h), rng, bad=0.02)
        x[0, 0, :3] = (1e-42, -3e-39, 3.0e38)
        x.view(np.uint32)[1, 1, 0] = 0x7FC01234          # a NaN with a payload
        got, want = ah.remodulate(x, g, L), dk.remodulate(x, g)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got[..., 3]), bits(x[..., 3]))
        low = (g[..., :3] < ak.FLOOR) & np.isfinite(x[..., :3])
        assert low.sum() >= 9 and np.array_equal(bits(got[..., :3][low]), bits((x[..., :3][low] * np.float32(ak.FLOOR)).astype(np.float32)))


def test_remodulation_is_the_denoisers():
    check_remodulation_is_the_denoisers()


def test_off_changes_no_bit():
    """with the adaptor absent nothing of this feature runs: the parent's host builds are compiled from headers this feature does not edit (pt_temporal.h,
    pt_svgf.h, pt_motion.h, pt_denoise.h carry no reference to pt_albedo.h), and an albedo of exactly 1 makes the adaptor the identity on every bit"""
    for header in ("pt_temporal.h", "pt_svgf.h", "pt_motion.h", "pt_denoise.h"):
        assert "albedo.h" not in open(os.path.join(ah.CSRC, header)).read()
    size = (45, 37)
    hist = None
    for k in range(2):
        inp = ak.call_inputs(size, "none", k)
        one = np.ones_like(inp["g0"])
        rc, new = ah.temporal(inp["colour"], one, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), hist, moments=True)
        old = None if hist is None else sh.History(hist.colour, hist.guide, hist.length, hist.moments, hist.world_to_clip, hist.eye)
        rc2, want = sh.temporal_m(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), old)
        assert rc == 0 == rc2 and same(new, want, True)
        hist = new


# ---- against the float64 model ---------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(err, bound, sel):
    with np.errstate(all="ignore"):
        r = np.where(sel, err / (bound * SLACK + 1e-300), 0.0)
    assert not np.isnan(r).any()
    return float(np.max(r, initial=0.0))


def step_ratios(inp, r, d, new, outcome=None):
    """worst error / bound of one call's colour and length on the kept pixels; a pixel without history holds the fp32 quotient bit for bit"""
    n = inp["w"] * inp["h"]
    k = r["kept"]
    fin = k & (r["outcome"] <= tk.HISTORY_ONLY)
    out, length = new.colour.reshape(n, 4)[:, :3].astype(np.float64), new.length.reshape(n).astype(np.float64)
    with np.errstate(invalid="ignore"):      # (Inf - Inf on pixels outside `fin`)
        err, err_n = np.abs(out - r["out"]), np.abs(length - r["length"])
    worst = {"out": worst_ratio(err, r["out_e"], fin[:, None] & np.ones(3, bool)), "length": worst_ratio(err_n, r["length_e"], fin)}
    plain = k & (r["outcome"] >= tk.CURRENT)
    assert np.array_equal(bits(new.colour.reshape(n, 4)[plain]), bits(d.astype(np.float32).reshape(n, 4)[plain])) and np.array_equal(length[plain], r["length"][plain])
    if outcome is not None:
        assert (outcome.reshape(n)[k] == r["outcome"][k]).all()
    return worst


def check_step_meets_model(size, move, L=None):
    """every call of the sequence with moments: colour, length and moments within the bound on the temporal model's kept pixels.  Returns the worst ratios"""
    worst = {}
    n = size[0] * size[1]
    calls = run_sequence(size, move, True, L)
    for k, (inp, hist, new) in enumerate(calls if move in ("none", "first") else calls[-1:]):
        jin = dict(inp, hist=None if hist is None else {"colour": hist.colour, "guide": hist.guide, "length": hist.length, "worldToClip": hist.world_to_clip, "eye": hist.eye})
        r, d = ak.judge_step(jin)
        assert 1 - r["kept"].mean() <= ak.DROP_CAP, (size, move, k)
        for name, v in step_ratios(jin, r, d, new).items():
            worst[name] = max(worst.get(name, 0.0), v)
        m, m_e, _ = ak.judge_moments(jin, None if hist is None else hist.moments)
        worst["moments"] = max(worst.get("moments", 0.0), worst_ratio(np.abs(new.moments.reshape(n, 2).astype(np.float64) - m), m_e, r["kept"][:, None] & np.ones(2, bool)))
        for (y, x) in inp["overflow"]:      # the overflowing quotient is a colour that is not finite, in the model as on the host
            assert r["outcome"][y * size[0] + x] in (tk.HISTORY_ONLY, tk.NOTHING)
    assert all(v <= 1.0 for v in worst.values()), f"{size} {move}: error / bound {worst}"
    return worst


@pytest.mark.parametrize("size,move", SEQ_CASES, ids=IDS(SEQ_CASES))
def test_step_meets_model(size, move):
    check_step_meets_model(size, move)


def check_moving_step_meets_model(size, move):
    inp = ak.motion_inputs(size, move)
    r, d = ak.judge_step(inp, mk.judge)
    assert 1 - r["kept"].mean() <= ak.DROP_CAP, (size, move)
    new, outcome, _ = run_moving(inp, False, moving_history(inp, False, None))
    worst = step_ratios(inp, r, d, new, outcome)
    assert all(v <= 1.0 for v in worst.values()), f"{size} {move}: error / bound {worst}"
    return worst


@pytest.mark.parametrize("size,move", MOTION_CASES, ids=IDS(MOTION_CASES))
def test_moving_step_meets_model(size, move):
    check_moving_step_meets_model(size, move)


def check_filtered_and_remodulated_meets_model(size, move, L=None):
    """pt_svgf_history on the demodulated history the sequence leaves: the last iteration judged from the host build's own input to it (section 5.4's model as
    it stands), times the albedo, within the grown bound; the variance is section 5.4's, in demodulated units"""
    n = size[0] * size[1]
    inp, _, hist = run_sequence(size, move, True)[-1]
    guides, prm = (inp["g0"], inp["g1"], inp["g2"]), sk.params()
    p = sh.params(int(prm["iterations"]), float(prm["sigmaLum"]), float(prm["lumFloor"]), tuple(float(v) for v in prm["sigmaGuide"]), float(prm["minTemporal"]))
    rc, v0, steps = sh.filter_history(sh.History(hist.colour, hist.guide, hist.length, hist.moments, hist.world_to_clip, hist.eye), guides, p)
    assert rc == 0
    c_in, v_in = (steps[-2] if len(steps) > 1 else (hist.colour, v0))
    r = sk.judge_iteration(c_in, v_in, guides, prm, len(steps) - 1)
    assert 1 - r["kept"].mean() <= ak.DROP_CAP
    want, want_e = ak.remodulated(r["out"], r["out_e"], inp["g0"])
    rc, got, var = ah.svgf_history(hist, guides, p, L)
    assert rc == 0 and np.array_equal(bits(var), bits(steps[-1][1]))
    judged = (r["kept"] & r["nz"])[:, None] & np.ones(3, bool)
    worst = worst_ratio(np.abs(got.reshape(n, 4)[:, :3].astype(np.float64) - want), want_e, judged)
    assert worst <= 1.0, f"{size} {move}: error / bound {worst}"
    return worst


@pytest.mark.parametrize("size,move", [(s, m) for s in SIZES for m in ("none", "yaw", "disocclude")], ids=lambda v: str(v).replace(" ", ""))
def test_filtered_and_remodulated_meets_model(size, move):
    check_filtered_and_remodulated_meets_model(size, move)


def test_the_fixture_meets_its_caps():
    """every case drops at most 5 % of its pixels (the temporal model's own mask, section 5.3's cap); the texture holds every planted value and no NaN, lies in
    [0.25, 1] otherwise; every case has its overflowing quotients, finite colours over albedo 0.001"""
    for size, move in SEQ_CASES:
        inp = ak.call_inputs(size, move, sk.calls_of(move) - 1)
        g = inp["g0"][..., :3]
        assert np.isfinite(inp["g0"]).all() and all((g == np.float32(v)).any() for v in ak.PLANTED)
        rest = ~np.isin(g, np.array(ak.PLANTED, np.float32))
        assert g[rest].min() >= 0.25 and g[rest].max() <= 1.0 and len(np.unique(g[rest])) > 0.9 * rest.sum()
        assert len(inp["overflow"]) == 4
        for (y, x) in inp["overflow"]:
            assert np.isfinite(inp["colour"][y, x, :3]).all() and not np.isfinite(ak.demodulate64(inp["colour"], inp["g0"])[y, x, :3]).all()
    for size, move in SEQ_CASES:
        for (inp, hist, _) in run_sequence(size, move, True)[-1:]:
            jin = dict(inp, hist=None if hist is None else {"colour": hist.colour, "guide": hist.guide, "length": hist.length, "worldToClip": hist.world_to_clip, "eye": hist.eye})
            assert 1 - ak.judge_step(jin)[0]["kept"].mean() <= ak.DROP_CAP, (size, move)


# ---- what it is for --------------------------------------------------------------------------------------------------------------------------------------------
W4, H4, CALLS4, NOISE4 = 96, 64, 8, 0.25


def flat_scene():
    """a static camera on constant guides: normal (0, 0, 1) encoded, depth 5"""
    cam = tk.moved("none", W4 / H4)
    g1 = np.zeros((H4, W4, 4), np.float32)
    g1[...] = (0.5, 0.5, 1.0, 1.0)
    g2 = np.zeros((H4, W4, 4), np.float32)
    g2[..., 0] = 5.0
    p = th.params(cam["worldToClip"], 0.05, 0.05, 64.0)
    return cam, g1, g2, p


def accumulate(albedo, seed, demodulated, L=None):
    """CALLS4 static calls of colour = albedo * (1 + NOISE4 * gaussian), through the demodulating step or through the parent's.  Returns the history"""
    cam, g1, g2, p = flat_scene()
    rng = np.random.default_rng(seed)
    hist = None
    for _ in range(CALLS4):
        c = np.ones((H4, W4, 4), np.float32)
        c[..., :3] = albedo[..., :3] * (1.0 + NOISE4 * rng.standard_normal((H4, W4, 1)))
        if demodulated:
            rc, hist = ah.temporal(c, albedo, g1, g2, cam["viewInverse"], cam["projInverse"], p, hist, moments=True, L=L)
        else:
            rc, hist = sh.temporal_m(c, g1, g2, cam["viewInverse"], cam["projInverse"], p, hist)
        assert rc == 0
    return hist, (g1, g2)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def filtered(hist, guides, sigma0, demodulated, L=None):
    p = sh.params(5, 4.0, 1e-4, (sigma0, 1.0, 1.0))
    if demodulated:
        rc, img, _ = ah.svgf_history(hist, guides, p, L)
        assert rc == 0
        return img
    rc, _, steps = sh.filter_history(hist, guides, p)
    assert rc == 0
    return steps[-1][0]


@pytest.mark.parametrize("seed", [400, 401])
def test_what_it_is_for_textured(seed):
    """a per-texel random albedo, illumination 1 with noise 0.25, 8 static calls, 5 iterations, plane 0 installed: the demodulated route with the albedo term
    out of action (sigmaGuide[0] = 1e15) ends below 0.25 x the BEST the undemodulated route reaches over sigmaGuide[0] in {0.02, 0.05, 0.1, 0.3, 1e15}, and
    below the unfiltered history.  Measured with the parent's code: 0.09 - 0.11 x; the margin covers the seed spread (about 10 %) and is the 0.25 of section
    5.4's edge test."""
    albedo = np.ones((H4, W4, 4), np.float32)
    level = np.random.default_rng(seed + 1000).uniform(0.25, 1.0, (H4, W4, 1)).astype(np.float32)
    albedo[..., :3] = level
    clean = albedo.copy()
    plain, (g1, g2) = accumulate(albedo, seed, False)
    demod, _ = accumulate(albedo, seed, True)
    guides = (albedo, g1, g2)
    best = min(rmse(filtered(plain, guides, s, False), clean) for s in (0.02, 0.05, 0.1, 0.3, 1e15))
    unfiltered = rmse(plain.colour, clean)
    ours = rmse(filtered(demod, guides, 1e15, True), clean)
    print(f"seed {seed}: demodulated {ours:.5f}, best undemodulated {best:.5f} ({ours / best:.3f} x), unfiltered history {unfiltered:.5f}")
    assert ours < 0.25 * best and ours < unfiltered


def check_checkerboard(seed, L=None):
    """a one-pixel checkerboard of albedo 0.5 / 0.625, no guide term: (contrast of the demodulated route, of the undemodulated one)"""
    albedo = np.ones((H4, W4, 4), np.float32)
    ys, xs = np.mgrid[0:H4, 0:W4]
    bright = (xs + ys) % 2 == 0
    albedo[..., :3] = np.where(bright, 0.625, 0.5)[..., None]
    plain, (g1, g2) = accumulate(albedo, seed, False)
    demod, _ = accumulate(albedo, seed, True, L)
    guides = (albedo, g1, g2)
    contrast = lambda img: float(img[..., :3][bright].astype(np.float64).mean() / img[..., :3][~bright].astype(np.float64).mean())   # noqa: E731
    ours, theirs = contrast(filtered(demod, guides, 1e15, True, L)), contrast(filtered(plain, guides, 1e15, False))
    print(f"seed {seed}: contrast demodulated {ours:.5f}, undemodulated {theirs:.5f}")
    assert abs(ours - 1.25) <= 0.005, ours
    assert theirs < 1.125, theirs
    return ours, theirs


@pytest.mark.parametrize("seed", [300, 301])
def test_what_it_is_for_checkerboard(seed):
    """mean output on bright texels over mean on dark ones within 0.005 of 1.25 (measured 1.2499 - 1.2500: the residual noise averages over 3072 texels per
    class); the undemodulated route stays below 1.125 -- it loses more than half the contrast (measured 1.03)"""
    check_checkerboard(seed)


# ---- refusals, each with its text --------------------------------------------------------------------------------------------------------------------------------
def check_refusals(L=None):
    for on in (0, 1):
        assert ah.refusal(ah.SETTING, on, L=L) == (capi.PT_OK, "")
    for on in (-1, 2, 255, 1 << 30):
        assert ah.refusal(ah.SETTING, on, L=L) == (capi.PT_ERR_INVALID, "on must be 0 or 1")
    for planes in range(8):
        have = planes & 1
        rc, why = ah.refusal(ah.STEP_NEEDS_PLANE, 1, planes, L=L)
        assert (rc, why) == ((capi.PT_OK, "") if have else (capi.PT_ERR_STATE, "pt_temporal_demodulate is on: guide plane 0 (the albedo) must be installed to divide by"))
        rc, why = ah.refusal(ah.NEED_PLANE, 1, planes, L=L)
        assert (rc, why) == ((capi.PT_OK, "") if have else (capi.PT_ERR_STATE, "the history is demodulated (pt_temporal_demodulate): guide plane 0 (the albedo) must be installed to multiply by"))
        assert ah.refusal(ah.STEP_NEEDS_PLANE, 0, planes, L=L) == (capi.PT_OK, "") == ah.refusal(ah.NEED_PLANE, 0, planes, L=L)
    assert ah.refusal(ah.DENOISE_FLAGS, 1, capi.PT_DENOISE_DEMODULATE, L=L) == (capi.PT_ERR_STATE, "PT_DENOISE_DEMODULATE on a history that is already demodulated (pt_temporal_demodulate)")
    assert ah.refusal(ah.DENOISE_FLAGS, 1, 0, L=L) == (capi.PT_OK, "") == ah.refusal(ah.DENOISE_FLAGS, 0, capi.PT_DENOISE_DEMODULATE, L=L)


def test_refusals_have_their_texts():
    """the setting's values, plane 0 missing at the step and at a consumer, PT_DENOISE_DEMODULATE on a demodulated history: pt_albedo.h states each once, the
    entry points prefix their name (tests/test_albedo_gpu.py reads them through the C ABI, with the state: a change drops the history, pt_resize keeps it)"""
    check_refusals()


def test_the_binding_names_the_setting():
    names = [n for n, _, _ in capi.API]
    assert "pt_temporal_demodulate" in names and "pt_debug_albedo_time" in [n for n, _, _ in capi.DEBUG_API]
    assert "int pt_temporal_demodulate(pt_context* ctx, int on);" in open(os.path.join(ROOT, "include", "pt_api.h")).read()
    assert "pt_debug_albedo_time" not in open(os.path.join(ROOT, "include", "pt_api.h")).read()
    from vk_raytrace_amd.renderer import HipRenderer
    assert callable(HipRenderer.temporal_demodulate)


# ---- planted breaks ----------------------------------------------------------------------------------------------------------------------------------------------
ALBEDO, UNIT, STEP, COMMON = "pt_albedo.h", "albedo_host.cpp", "stage/history_step.h", "stage/stage_host_common.h"
BREAKS = {
    "moments_from_the_raw_colour": ([(STEP, "svgf_moments(msrc, pr, o, src.colour(x, y));", "svgf_moments(msrc, pr, o, ((const DnPx*)q.colour)[at]);")],
                                    lambda L: check_composition_static((45, 37), "none", True, L)),
    "remodulation_at_the_history_position": ([(UNIT, "std::memcpy(&g, albedo + 4 * i, sizeof(DnPx));", "std::memcpy(&g, albedo + 4 * (i + 1 < n ? i + 1 : i), sizeof(DnPx));")],
                                             lambda L: check_checkerboard(300, L)),
    "floor_missing": ([(ALBEDO, "PT_DN DnPx albedo_remodulate(const DnPx& x, const DnPx& g) { return denoise_remodulate(x, g); }",
                        "PT_DN DnPx albedo_remodulate(const DnPx& x, const DnPx& g) { return DnPx{dn_finite(x.x) ? x.x * g.x : x.x, dn_finite(x.y) ? x.y * g.y : x.y, dn_finite(x.z) ? x.z * g.z : x.z, x.w}; }")],
                      lambda L: check_remodulation_is_the_denoisers(L)),
    "remodulating_twice": ([(ALBEDO, "{ return denoise_remodulate(x, g); }", "{ return denoise_remodulate(denoise_remodulate(x, g), g); }")], lambda L: check_checkerboard(300, L)),
    "demodulating_the_gathered_taps": ([(ALBEDO, "DnPx histColour(int x, int y) const { return src.histColour(x, y); }",
                                         "DnPx histColour(int x, int y) const { return denoise_demodulate(src.histColour(x, y), src.albedo(x, y)); }")],
                                       lambda L: check_composition_static((45, 37), "none", False, L)),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_a_planted_break_fails_its_test(name):
    edits, check = BREAKS[name]
    with tempfile.TemporaryDirectory() as tmp:
        os.mkdir(os.path.join(tmp, "stage"))       # the unit's own headers go next to its copy
        for fname, src_dir in ((ALBEDO, ah.CSRC), (UNIT, os.path.join(ROOT, "tests", "cpp")), (STEP, os.path.join(ROOT, "tests", "cpp")), (COMMON, os.path.join(ROOT, "tests", "cpp"))):
            text = open(os.path.join(src_dir, fname)).read()
            for _, old, new in [e for e in edits if e[0] == fname]:
                assert text.count(old) == 1, (name, old)
                text = text.replace(old, new)
            open(os.path.join(tmp, fname), "w").write(text)
        import subprocess
        out = os.path.join(tmp, "libbroken.so")
        subprocess.check_call(["g++", "-I" + tmp] + ah.COMPILE + ["-shared", "-o", out, os.path.join(tmp, UNIT)])
        L = ah.bind(out)
        with pytest.raises(AssertionError):
            check(L)

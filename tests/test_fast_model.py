"""The responsive history: the host build of vk_raytrace_amd/csrc/pt_fast.h behind the temporal steps (tests/fast_host.py) against
the parent's host builds, bit for bit; against the float64 model (tests/golden/gen_fast_kat.py); exact cases; what the feature is for; its refusals;
planted breaks; the stand-alone program under the sanitizers.  No GPU: tests/test_fast_gpu.py holds the device to this host build bit for bit, and the
context's state (the setting, the history's mark) to the definition.

Composition.  The fast step is the parent's step over other planes: Hf' and Hnf' have to be what temporal_host / motion_host / albedo_host give from
(Hf, Hg, Hnf) with maxHistory = maxFast, on every bit; with sigmaScale = 1e6 nothing clamps on the fixtures and Hc', Hn' and Hm' have to be the parent's.

The bound against the model is section 5.3's running first-order bound carried through the clamp's statements (gen_fast_kat's docstring derives it),
applied as it stands with the 2^-20 slack of tests/test_temporal_model.py.  measure_fast_kat.py records the worst ratio in fast_kat_tol.json: reported,
not used.  A case may drop at most 5 % of its pixels from the Hn' judgement.

Planted breaks (test_a_planted_break_fails_its_test applies each to scratch copies of the header or of the host build's unit, never to the tree):
    the clamp reads Hf of the read set           step_is_two_steps_then_the_clamp
    sigma without the max with 0                 negative_variance_counts_as_zero
    the length is not cut                        length_is_cut_where_a_channel_moved
    the length is cut at every pixel             length_is_cut_where_a_channel_moved
    the fast step runs with maxHistory           composition_static
    a skipped tap is still counted in n          hostile_planes
    demodulating: the fast step reads c raw      composition_static (demodulated)
"""
import importlib.util
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import albedo_host as ah, fast_host as fh, motion_host as mh, svgf_host as sh, temporal_host as th
from tests import test_temporal_model as tmodel
from vk_raytrace_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_fast_kat", os.path.join(ROOT, "tests", "golden", "gen_fast_kat.py"))
fk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fk)
ak, sk, mk, dk, tk = fk.ak, fk.sk, fk.mk, fk.dk, fk.tk
bits, SLACK = tmodel.bits, tmodel.SLACK
SIZES = tk.SIZES
SEQ_MOVES = ("none", "yaw", "disocclude", "first")
SEQ_CASES = [(size, move) for size in SIZES for move in SEQ_MOVES]
MOTION_CASES = [(size, "slide") for size in SIZES]
IDS = lambda cases: [f"{s[0]}x{s[1]}-{m}" for s, m in cases]   # noqa: E731
ASAN_MAIN = os.path.join(ROOT, "tests", "cpp", "fast_asan_main.cpp")
NEVER = 1.0e6   # a sigmaScale under which nothing clamps on the fixtures


def fast_params(prm=None, **over):
    prm = dict(fk.FAST if prm is None else prm, **over)
    return fh.params(float(prm["maxFast"]), float(prm["sigmaScale"]), int(prm["radius"]))


def params_of(inp, max_history=None):
    return th.params(inp["worldToClip"], float(inp["depthTol"]), float(inp["normalDist2"]), float(inp["maxHistory"] if max_history is None else max_history))


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """equal bit for bit, or NaN on both sides"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the sequences on the new host build ---------------------------------------------------------------------------------------------------------------------
_sequences = {}


def inputs_of(size, move, k, demod):
    return ak.call_inputs(size, move, k) if demod else sk.call_inputs(size, move, k)


def run_sequence(size, move, moments, demod, fp=None, L=None):
    """the calls of a case on the new host build, each fed the one before: [(inputs, the history read or None, the history written)]"""
    out, hist = [], None
    fp = fp or fast_params()
    for k in range(sk.calls_of(move)):
        key = (size, k if k < sk.STATIC_CALLS else move, moments, demod, fp.maxFast, fp.sigmaScale, fp.radius)
        if L is None and key in _sequences:
            out.append(_sequences[key])
        else:
            inp = inputs_of(size, move, k, demod)
            rc, new = fh.step(inp["colour"], inp["g0"] if demod else None, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), fp, hist, moments=moments, L=L)
            assert rc == 0
            out.append((inp, hist, new))
            if L is None:
                _sequences[key] = out[-1]
        hist = out[-1][2]
    return out


def as_fast(hist):
    """the fast images of a history as a history of their own, for the parent's host builds"""
    return None if hist is None else mh.History(hist.fast, hist.guide, hist.fast_length, hist.world_to_clip, hist.eye)


# ---- composition, bit for bit ---------------------------------------------------------------------------------------------------------------------------------
def parent_step(inp, p, hist, demod, moments=False):
    """the parent's host build of the step the settings select, static form"""
    if demod:
        rc, want = ah.temporal(inp["colour"], inp["g0"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, hist, moments=moments)
    elif moments:
        old = None if hist is None else sh.History(hist.colour, hist.guide, hist.length, hist.moments, hist.world_to_clip, hist.eye)
        rc, want = sh.temporal_m(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, old)
    else:
        rc, want = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, hist)
    assert rc == 0
    return want


def check_composition_static(size, move, moments, demod, L=None):
    """every call of the sequence: Hf', Hnf' are the parent's host build with maxHistory = maxFast on (Hf, Hg, Hnf); the colour before the clamp is the
    parent's long step; and under a sigmaScale that never clamps the stored Hc', Hn', Hm' are the parent's as well"""
    fp = fast_params()
    for k, (inp, hist, new) in enumerate(run_sequence(size, move, moments, demod, fp, L)):
        what = f"{size} {move} call {k} moments {moments} demodulated {demod}"
        want = parent_step(inp, params_of(inp, fp.maxFast), as_fast(hist), demod)
        assert same(new.fast, want.colour) and same(new.fast_length, want.length) and same(new.guide, want.guide), f"{what}: the fast step is not the parent's with maxFast"
        long = parent_step(inp, params_of(inp), hist, demod, moments)
        assert same(new.raw, long.colour) and same(new.raw_length, long.length) and same(new.guide, long.guide), f"{what}: the long step is not the parent's"
        assert not moments or same(new.moments, long.moments), f"{what}: the moments are not the parent's"
    hist = plain = None
    never = fast_params(sigmaScale=NEVER)
    for k in range(sk.calls_of(move)):
        inp = inputs_of(size, move, k, demod)
        rc, hist = fh.step(inp["colour"], inp["g0"] if demod else None, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), never, hist, moments=moments, L=L)
        plain = parent_step(inp, params_of(inp), plain, demod, moments)
        assert rc == 0 and same(hist.colour, plain.colour) and same(hist.length, plain.length) and (not moments or same(hist.moments, plain.moments)), f"call {k}: sigmaScale 1e6 clamped"


@pytest.mark.parametrize("demod", [False, True], ids=["raw", "demodulated"])
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size,move", SEQ_CASES, ids=IDS(SEQ_CASES))
def test_composition_static(size, move, moments, demod):
    check_composition_static(size, move, moments, demod)


def moving_inputs(size, move, demod):
    inp = ak.motion_inputs(size, move) if demod else mk.case_inputs(size, move)
    hf, hnf = fk.fast_history_for(inp, size[0])
    H = inp["hist"]
    hm = np.exp(np.random.default_rng(5).uniform(-3, 3, (inp["h"], inp["w"], 2))).astype(np.float32)
    return inp, fh.History(H["colour"], H["guide"], H["length"], H["worldToClip"], H["eye"], hm, hf, hnf)


def run_moving(inp, hist, moments, demod, fp, L=None):
    tab = None if hist is None else mh.table(inp["hist_words"], inp["cur_words"])
    rc, new = fh.step(inp["colour"], inp["g0"] if demod else None, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), fp, hist, moments=moments,
                      ids=inp["ids"], tab=tab, L=L)
    assert rc == 0
    return new, tab


@pytest.mark.parametrize("demod", [False, True], ids=["raw", "demodulated"])
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size,move", MOTION_CASES, ids=IDS(MOTION_CASES))
def test_composition_moving(size, move, moments, demod):
    """the moving form: a first call, then the move on the fixture's history"""
    inp, fixture = moving_inputs(size, move, demod)
    fp = fast_params()
    for hist in (None, fixture):
        new, tab = run_moving(inp, hist, moments, demod, fp)
        for maxh, h0, got, got_n in ((fp.maxFast, as_fast(hist), new.fast, new.fast_length), (None, hist, new.raw, new.raw_length)):
            m = moments and maxh is None
            if demod:
                rc, want = ah.temporal(inp["colour"], inp["g0"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp, maxh), h0, moments=m, ids=inp["ids"], tab=tab)
            else:
                rc, want = mh.temporal_moving(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp, maxh), inp["ids"], tab, h0, moments=m)
            assert rc == 0 and same(got, want.colour) and same(got_n, want.length) and same(new.guide, want.guide), f"{size} {move}: history {hist is not None}, maxHistory {maxh}"
            assert not m or same(new.moments, want.moments)


def check_step_is_two_steps_then_the_clamp(L=None):
    """what a call stores is the clamp of what its long step wrote against what its fast step WROTE (Hf', Hnf': not the set that was read), and the
    moments are the long step's"""
    size, fp = (45, 37), fast_params()
    moved = 0
    for inp, hist, new in run_sequence(size, "yaw", True, False, fp, L):
        rc, c, n = fh.clamp(new.fast, new.fast_length, new.raw, new.raw_length, fp)
        assert rc == 0 and same(new.colour, c) and same(new.length, n)
        moved += int((bits(new.colour) != bits(new.raw)).any(-1).sum())
        assert same(new.colour[..., 3], new.raw[..., 3])
    assert moved > 500


def test_step_is_two_steps_then_the_clamp():
    check_step_is_two_steps_then_the_clamp()


# ---- against the float64 model ---------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(err, bound, sel):
    with np.errstate(all="ignore"):
        r = np.where(sel, err / (bound * SLACK + 1e-300), 0.0)
    assert not np.isnan(r).any()
    return float(np.max(r, initial=0.0))


def clamp_ratios(new, prm, what, L=None):
    """the clamp of one call judged from the host build's own step outputs: mu, sigma, lo, hi and the clamped colour within the bound on the kept pixels,
    Hn' equal on the pixels kept for it, at most 5 % dropped.  Returns the worst ratios"""
    h, w = new.length.shape
    n = w * h
    r = fk.judge_clamp(new.fast, new.fast_length, new.raw, new.raw_length, prm)
    dropped = 1 - r["kept_n"].mean()
    assert dropped <= fk.DROP_CAP, f"{what}: {100 * dropped:.2f} % of the pixels dropped from the Hn' judgement"
    fp = fast_params(prm)
    rc, c, ln, pr = fh.clamp(new.fast, new.fast_length, new.raw, new.raw_length, fp, want_probe=True, L=L)
    assert rc == 0
    kept3 = (r["kept"] & r["enough"])[:, None] & np.ones(3, bool)
    worst = {}
    for name in ("mu", "sigma", "lo", "hi"):
        with np.errstate(invalid="ignore"):
            worst[name] = worst_ratio(np.abs(pr[name].reshape(n, 3).astype(np.float64) - r[name]), r[name + "_e"], kept3)
    with np.errstate(invalid="ignore"):      # (Inf - Inf on pixels that are not touched)
        worst["out"] = worst_ratio(np.abs(c.reshape(n, 4)[:, :3].astype(np.float64) - r["out"]), r["out_e"], (r["kept"] & r["touched"])[:, None] & np.ones(3, bool))
    untouched = r["kept"] & ~r["touched"]
    assert same(c.reshape(n, 4)[untouched], new.raw.reshape(n, 4)[untouched]) and same(c[..., 3], new.raw[..., 3])
    assert np.array_equal(ln.reshape(n)[r["kept_n"]].astype(np.float64), r["length"][r["kept_n"]]), f"{what}: Hn' differs from the model on pixels kept for it"
    assert (pr["moved"].reshape(n)[r["kept_n"]] == r["moved"][r["kept_n"]]).all()
    assert np.array_equal(pr["n"].reshape(n).astype(np.float64), r["n"])
    assert r["moved"][r["kept_n"]].sum() > 0.05 * n and (~r["moved"] & r["touched"])[r["kept_n"]].sum() > 0.05 * n, f"{what}: both branches of Hn' must be filled"
    assert (r["sigma"][r["enough"] & r["kept"]] > 0).all(), f"{what}: the fixture's noise keeps sigma > 0 wherever n >= 2"
    assert all(v <= 1.0 for v in worst.values()), f"{what}: error / bound {worst}"
    return worst


def check_clamp_meets_model(size, move, demod, prm=None, L=None):
    worst = {}
    prm = prm or fk.FAST
    calls = run_sequence(size, move, False, demod, fast_params(prm), L)
    for k, (inp, hist, new) in enumerate(calls if move in ("none", "first") else calls[-1:]):
        for name, v in clamp_ratios(new, prm, f"{size} {move} call {k}", L).items():
            worst[name] = max(worst.get(name, 0.0), v)
    return worst


@pytest.mark.parametrize("demod", [False, True], ids=["raw", "demodulated"])
@pytest.mark.parametrize("size,move", SEQ_CASES, ids=IDS(SEQ_CASES))
def test_clamp_meets_model(size, move, demod):
    check_clamp_meets_model(size, move, demod)


@pytest.mark.parametrize("radius", [1, 3])
def test_clamp_meets_model_at_other_radii(radius):
    check_clamp_meets_model((45, 37), "yaw", False, dict(fk.FAST, radius=radius))


def check_fast_step_meets_model(size, move, demod):
    """Hf', Hnf' of the last call of the sequence within the bound of the imported model run on (Hf, Hg, Hnf) with maxFast; the long step's colour before
    the clamp within the bound of the same model as it stands.  Returns the worst ratios"""
    inp, hist, new = run_sequence(size, move, False, demod)[-1]
    n = size[0] * size[1]
    jin = dict(inp, hist=None if hist is None else {"colour": hist.colour, "guide": hist.guide, "length": hist.length, "worldToClip": hist.world_to_clip, "eye": hist.eye})
    long, fast = fk.step_models(jin, None if hist is None else (hist.fast, hist.fast_length), fk.FAST, demod)
    worst = {}
    for name, r, colour, length in (("long", long, new.raw, new.raw_length), ("fast", fast, new.fast, new.fast_length)):
        assert 1 - r["kept"].mean() <= fk.DROP_CAP, (size, move, name)
        sel = r["kept"] & (r["outcome"] <= tk.HISTORY_ONLY)
        with np.errstate(invalid="ignore"):
            err, err_n = np.abs(colour.reshape(n, 4)[:, :3].astype(np.float64) - r["out"]), np.abs(length.reshape(n).astype(np.float64) - r["length"])
        worst[name] = worst_ratio(err, r["out_e"], sel[:, None] & np.ones(3, bool))
        worst[name + "_length"] = worst_ratio(err_n, r["length_e"], sel)
    assert all(v <= 1.0 for v in worst.values()), f"{size} {move}: error / bound {worst}"
    return worst


@pytest.mark.parametrize("demod", [False, True], ids=["raw", "demodulated"])
@pytest.mark.parametrize("size,move", [(s, m) for s in SIZES for m in ("none", "yaw")], ids=lambda v: str(v).replace(" ", ""))
def test_fast_step_meets_model(size, move, demod):
    check_fast_step_meets_model(size, move, demod)


def check_moving_meets_model(size, move, demod):
    inp, fixture = moving_inputs(size, move, demod)
    new, _ = run_moving(inp, fixture, False, demod, fast_params())
    n = size[0] * size[1]
    long, fast = fk.step_models(inp, (fixture.fast, fixture.fast_length), fk.FAST, demod, mk.judge)
    worst = {}
    for name, r, colour in (("long", long, new.raw), ("fast", fast, new.fast)):
        assert 1 - r["kept"].mean() <= fk.DROP_CAP
        sel = r["kept"] & (r["outcome"] <= tk.HISTORY_ONLY)
        with np.errstate(invalid="ignore"):
            worst[name] = worst_ratio(np.abs(colour.reshape(n, 4)[:, :3].astype(np.float64) - r["out"]), r["out_e"], sel[:, None] & np.ones(3, bool))
    # (the fixture's colours are log-uniform over four decades: the window's spread is of the order of its mean and few pixels clamp at sigmaScale 1)
    r = fk.judge_clamp(new.fast, new.fast_length, new.raw, new.raw_length, fk.FAST)
    assert 1 - r["kept_n"].mean() <= fk.DROP_CAP
    kept3 = (r["kept"] & r["touched"])[:, None] & np.ones(3, bool)
    with np.errstate(invalid="ignore"):
        worst["out"] = worst_ratio(np.abs(new.colour.reshape(n, 4)[:, :3].astype(np.float64) - r["out"]), r["out_e"], kept3)
    assert np.array_equal(new.length.reshape(n)[r["kept_n"]].astype(np.float64), r["length"][r["kept_n"]])
    assert all(v <= 1.0 for v in worst.values()), f"{size} {move}: error / bound {worst}"
    return worst


@pytest.mark.parametrize("demod", [False, True], ids=["raw", "demodulated"])
@pytest.mark.parametrize("size,move", MOTION_CASES, ids=IDS(MOTION_CASES))
def test_moving_meets_model(size, move, demod):
    check_moving_meets_model(size, move, demod)


# ---- exact cases -------------------------------------------------------------------------------------------------------------------------------------------------
def noisy_planes(w, h, seed, level=1.0):
    """(Hf', Hnf', Hc', Hn'): colours of `level` with 25 % noise, alpha 1; lengths 1 .. 8 (long) and 1 .. 4 (fast)"""
    rng = np.random.default_rng(seed)
    hf, hc = np.ones((h, w, 4), np.float32), np.ones((h, w, 4), np.float32)
    hf[..., :3] = level * (1.0 + 0.25 * rng.standard_normal((h, w, 3)))
    hc[..., :3] = level * (1.0 + 0.25 * rng.standard_normal((h, w, 3)))
    hc[..., 3] = rng.uniform(size=(h, w))
    return hf, rng.integers(1, 5, (h, w)).astype(np.float32), hc, rng.integers(1, 9, (h, w)).astype(np.float32)


def check_model32_is_the_host_build(planes, fp, L=None):
    """the model's float32 run and the host build: the same bits in every plane the probe hands out (no exponential is involved).  Returns both"""
    prm = {"maxFast": fp.maxFast, "sigmaScale": fp.sigmaScale, "radius": fp.radius}
    r = fk.clamp(*planes, prm, np.float32)
    rc, c, n, pr = fh.clamp(*planes, fp, want_probe=True, L=L)
    h, w = n.shape
    assert rc == 0
    assert same_values(c[..., :3].reshape(-1, 3), r["out"]) and same(c[..., 3], planes[2][..., 3]) and same_values(n.reshape(-1), r["length"])
    assert np.array_equal(pr["n"].reshape(-1), r["n"]) and np.array_equal(pr["moved"].reshape(-1) != 0, r["moved"])
    for name in ("mu", "sigma", "lo", "hi"):
        assert same_values(pr[name].reshape(-1, 3), r[name]), name
    return (c, n, pr), r


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", [(45, 37), (1, 1), (3, 200), (7, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_model32_is_the_host_build(size, radius):
    """this pins the tap order: fp32 sums in another order round otherwise"""
    check_model32_is_the_host_build(noisy_planes(*size, 31 + radius), fh.params(3.0, 1.0, radius))


def test_constant_fast_history_clamps_to_the_mean():
    """a constant Hf' (values whose sums and squares are exact in fp32) has sigma = 0: every pixel's colour becomes mu, which is the constant, bit for bit,
    and its length min(Hn', maxFast); a pixel that already holds the constant is not moved and keeps its length"""
    w, h = 21, 13
    hf, hnf, hc, hn = noisy_planes(w, h, 7)
    hf[..., :3] = (0.5, 2.0, 3.0)
    hc[4, 5, :3] = (0.5, 2.0, 3.0)
    hn[4, 5] = 8.0
    for radius in (1, 2, 3):
        for k in (0.0, 2.0, 1e6):
            rc, c, n, pr = fh.clamp(hf, hnf, hc, hn, fh.params(3.0, k, radius), want_probe=True)
            assert rc == 0 and (pr["sigma"] == 0).all() and same(pr["mu"], hf[..., :3]) and same(c[..., :3], hf[..., :3]) and same(c[..., 3], hc[..., 3])
            want_n = np.minimum(hn, 3.0)
            want_n[4, 5] = 8.0
            assert same(n, want_n) and pr["moved"].sum() == w * h - 1


def test_corner_and_single_pixel_counts():
    """radius 1 at the corner pixel has n = 4 (edge 6, inside 9); radius R inside has (2 R + 1)^2; a 1 x 1 image has n = 1 and is left untouched"""
    hf, hnf, hc, hn = noisy_planes(9, 8, 3)
    rc, _, _, pr = fh.clamp(hf, hnf, hc, hn, fh.params(3.0, 1.0, 1), want_probe=True)
    assert rc == 0 and pr["n"][0, 0] == 4 and pr["n"][7, 8] == 4 and pr["n"][0, 3] == 6 and pr["n"][3, 0] == 6 and pr["n"][3, 3] == 9
    for radius in (2, 3):
        rc, _, _, pr = fh.clamp(hf, hnf, hc, hn, fh.params(3.0, 1.0, radius), want_probe=True)
        assert pr["n"][4, 4] == (2 * radius + 1) ** 2
        assert pr["n"][0, 0] == (radius + 1) ** 2
    one = noisy_planes(1, 1, 4)
    one[2][0, 0, :3] = (50.0, -50.0, 0.0)
    for radius in (1, 2, 3):
        rc, c, n, pr = fh.clamp(*one, fh.params(1.0, 0.0, radius), want_probe=True)
        assert rc == 0 and pr["n"][0, 0] == 1 and same(c, one[2]) and same(n, one[3]) and np.isnan(pr["mu"]).all()


def check_length_is_cut_where_a_channel_moved(L=None):
    """Hn' = min(Hn', maxFast) exactly where a channel moved, and untouched everywhere else: both classes hold pixels whose length exceeds maxFast"""
    hf, hnf, hc, hn = noisy_planes(45, 37, 11)
    fp = fh.params(3.0, 1.0, 2)
    rc, c, n = fh.clamp(hf, hnf, hc, hn, fp, L=L)
    assert rc == 0
    moved = (bits(c) != bits(hc)).any(-1)
    longer = hn > 3.0
    assert (moved & longer).sum() > 100 and (~moved & longer).sum() > 100 and (moved & ~longer).sum() > 100
    assert same(n[moved], np.minimum(hn[moved], np.float32(3.0))) and same(n[~moved], hn[~moved])


def test_length_is_cut_where_a_channel_moved():
    check_length_is_cut_where_a_channel_moved()


def find_negative_variance():
    """a constant whose fp32 sums round so that s2 / n - mu mu comes out below 0 at an inside pixel of a 5 x 5 window"""
    for i in range(1, 4000):
        f = np.float32(0.1) + np.float32(i) * np.float32(0.001)
        s1 = s2 = np.float32(0)
        for _ in range(25):
            s1, s2 = np.float32(s1 + f), np.float32(s2 + np.float32(f * f))
        mu = np.float32(s1 / np.float32(25))
        if np.float32(np.float32(s2 / np.float32(25)) - np.float32(mu * mu)) < 0:
            return f, mu
    raise AssertionError("no such constant")


def check_negative_variance_counts_as_zero(L=None):
    """v < 0 by rounding is sigma = 0, not the square root of a negative number: the pixel is clamped to mu (a NaN bound would leave it untouched)"""
    f, mu = find_negative_variance()
    hf, hnf, hc, hn = noisy_planes(9, 9, 5)
    hf[..., :3] = f
    rc, c, n, pr = fh.clamp(hf, hnf, hc, hn, fh.params(2.0, 2.0, 2), want_probe=True, L=L)
    assert rc == 0 and pr["n"][4, 4] == 25 and (pr["sigma"][4, 4] == 0).all() and same(pr["mu"][4, 4], np.full(3, mu, np.float32))
    assert same(c[4, 4, :3], np.full(3, mu, np.float32)) and n[4, 4] == min(hn[4, 4], 2.0)


def test_negative_variance_counts_as_zero():
    check_negative_variance_counts_as_zero()


def hostile_planes(w, h, seed):
    """noisy planes with NaN, +-Inf and 3e38 channels planted in Hf' and Hc', lengths of 0, -1, NaN and 0.5 in Hnf' and Hn'.  Returns (planes, where Hf' or
    Hnf' is hostile (h, w), where Hc' or Hn' is)"""
    hf, hnf, hc, hn = noisy_planes(w, h, seed)
    rng = np.random.default_rng(seed + 1)
    bad_f, bad_c = np.zeros((h, w), bool), np.zeros((h, w), bool)
    values = np.array([np.nan, np.inf, -np.inf, 3.0e38, -3.0e38], np.float32)
    for plane, length, mark in ((hf, hnf, bad_f), (hc, hn, bad_c)):
        for _ in range(max(2, w * h // 40)):
            y, x = int(rng.integers(h)), int(rng.integers(w))
            plane[y, x, int(rng.integers(3))] = values[int(rng.integers(len(values)))]
            mark[y, x] = True
        for _ in range(max(2, w * h // 40)):
            y, x = int(rng.integers(h)), int(rng.integers(w))
            length[y, x] = (0.0, -1.0, np.nan, 0.5)[int(rng.integers(4))]
            mark[y, x] = True
    return (hf, hnf, hc, hn), bad_f, bad_c


def check_hostile_planes(L=None):
    """NaN, +-Inf, 3e38 (whose square overflows: hi is not finite and the pixel is left untouched) and lengths below 1: the host build is the model's float32
    run on every bit; a hostile pixel of Hc' / Hn' changes no other pixel, one of Hf' / Hnf' none outside its window; Hnf' = 0 everywhere touches nothing"""
    for (w, h), radius in (((45, 37), 2), ((17, 9), 3), ((3, 40), 1)):
        fp = fh.params(3.0, 1.5, radius)
        planes, bad_f, bad_c = hostile_planes(w, h, 50 + radius)
        (c, n, pr), r = check_model32_is_the_host_build(planes, fp, L)
        clean = noisy_planes(w, h, 50 + radius)
        rc, c0, n0 = fh.clamp(*clean, fp, L=L)
        ys, xs = np.mgrid[0:h, 0:w]
        reach = np.zeros((h, w), bool)
        for y, x in zip(*np.nonzero(bad_f)):
            reach |= (np.abs(ys - y) <= radius) & (np.abs(xs - x) <= radius)
        far = ~reach & ~bad_c
        assert far.sum() > 0 or w < 8
        assert same(c[far], c0[far]) and same(n[far], n0[far])
        own_bad = ~(planes[3] >= 1) | ~np.isfinite(planes[2][..., :3]).all(-1)
        assert same(c[own_bad], planes[2][own_bad]) and same(n[own_bad], planes[3][own_bad])                # left as they are, payload and all
        assert pr["n"][~own_bad].max() <= (2 * radius + 1) ** 2 and (pr["n"][reach & ~own_bad] < (2 * radius + 1) ** 2).any()
        big = np.abs(planes[0][..., :3]).max(-1) == np.float32(3.0e38)
        if big.any():                                                                                            # 3e38 counts as a tap; its square overflows
            y, x = [int(v[0]) for v in np.nonzero(big)]
            assert not np.isfinite(pr["hi"][y, x]).all() or own_bad[y, x] or planes[1][y, x] < 1 or not np.isfinite(planes[0][y, x, :3]).all()
        rc, c1, n1 = fh.clamp(planes[0], np.zeros_like(planes[1]), planes[2], planes[3], fp, L=L)
        assert rc == 0 and same(c1, planes[2]) and same(n1, planes[3])


def test_hostile_planes():
    check_hostile_planes()


def test_overflowing_square_leaves_the_pixel():
    """one tap of 3e38 among ordinary ones: it is finite and counts, s2 / n and mu mu both overflow, v is NaN and so is hi: every pixel whose window holds
    it is left untouched (and not clamped to a mean of 1e37)"""
    hf, hnf, hc, hn = noisy_planes(11, 11, 9)
    hf[5, 5, 1] = 3.0e38
    rc, c, n, pr = fh.clamp(hf, hnf, hc, hn, fh.params(2.0, 1.0, 2), want_probe=True)
    assert rc == 0 and pr["n"][5, 5] == 25 and (~np.isfinite(pr["hi"][3:8, 3:8, 1])).all() and np.isfinite(pr["mu"][3:8, 3:8, 1]).all()
    assert same(c[3:8, 3:8], hc[3:8, 3:8]) and same(n[3:8, 3:8], hn[3:8, 3:8]) and (bits(c[:2]) != bits(hc[:2])).any()


# ---- what it is for --------------------------------------------------------------------------------------------------------------------------------------------
W4 = H4 = 64
SWITCH, AFTER, MAX_HISTORY = 32, 8, 32.0
FOR = {"maxFast": 4.0, "sigmaScale": 2.0, "radius": 2}


def flat_scene():
    """a static camera on constant guides: normal (0, 0, 1) encoded, depth 5"""
    cam = tk.moved("none", W4 / H4)
    g1 = np.zeros((H4, W4, 4), np.float32)
    g1[...] = (0.5, 0.5, 1.0, 1.0)
    g2 = np.zeros((H4, W4, 4), np.float32)
    g2[..., 0] = 5.0
    return cam, g1, g2, th.params(cam["worldToClip"], 0.05, 0.05, MAX_HISTORY)


def rmse(a, level):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - level) ** 2)))


def host_response(seed, L=None):
    """SWITCH calls of illumination 1 with 25 % noise, then AFTER calls of illumination 3, through the clamped route (fast_host) and the parent's
    (temporal_host) on the same frames.  Returns {call: (clamped rmse, parent rmse, mean clamped Hn')} for the call before the switch and the last one"""
    cam, g1, g2, p = flat_scene()
    fp = fast_params(FOR)
    rng = np.random.default_rng(seed)
    ours = theirs = None
    out = {}
    for t in range(SWITCH + AFTER):
        level = 1.0 if t < SWITCH else 3.0
        c = np.ones((H4, W4, 4), np.float32)
        c[..., :3] = level * (1.0 + 0.25 * rng.standard_normal((H4, W4, 1)))
        rc, ours = fh.step(c, None, g1, g2, cam["viewInverse"], cam["projInverse"], p, fp, ours, L=L)
        rc2, theirs = th.temporal(c, g1, g2, cam["viewInverse"], cam["projInverse"], p, theirs)
        assert rc == 0 == rc2
        if t in (SWITCH - 1, SWITCH + AFTER - 1):
            out[t] = (rmse(ours.colour, level), rmse(theirs.colour, level), float(ours.length.mean()))
    return out


def model_response(seed=0):
    a = fk.response(SWITCH + AFTER, SWITCH, MAX_HISTORY, FOR, W4, H4, seed=seed)
    b = fk.response(SWITCH + AFTER, SWITCH, MAX_HISTORY, FOR, W4, H4, seed=seed, clamped=False)
    return {t: (a[t][0], b[t][0], a[t][1]) for t in (SWITCH - 1, SWITCH + AFTER - 1)}


@pytest.mark.parametrize("seed", [500, 501])
def test_what_it_is_for(seed):
    """Speed of response: 8 calls after the switch the clamped route's RMSE against the new clean image, over the parent's on the same frames, is below
    1.25 x the ratio the float64 model shows (recorded in fast_kat_tol.json) and below 0.5 in any case.  Cost when nothing changes: at call 32 the
    clamped RMSE is at most 1.1 x the parent's and the mean Hn' above 0.9 maxHistory.  The model alone meets both as well."""
    recorded = json.load(open(fk.TOL_PATH))["response"]
    model = model_response()
    m_ratio = model[SWITCH + AFTER - 1][0] / model[SWITCH + AFTER - 1][1]
    assert abs(m_ratio - recorded["ratio_after_8"]) < 1e-6, "fast_kat_tol.json is stale (measure_fast_kat.py)"
    assert m_ratio < 0.5 and model[SWITCH - 1][0] <= 1.1 * model[SWITCH - 1][1] and model[SWITCH - 1][2] > 0.9 * MAX_HISTORY
    host = host_response(seed)
    late, calm = host[SWITCH + AFTER - 1], host[SWITCH - 1]
    print(f"seed {seed}: 8 calls after the switch clamped {late[0]:.4f}, parent {late[1]:.4f} ({late[0] / late[1]:.3f} x; model {m_ratio:.3f} x); "
          f"call 32 clamped {calm[0]:.4f}, parent {calm[1]:.4f} ({calm[0] / calm[1]:.3f} x), mean Hn' {calm[2]:.2f}")
    assert late[0] / late[1] < 1.25 * m_ratio and late[0] / late[1] < 0.5
    assert calm[0] <= 1.1 * calm[1] and calm[2] > 0.9 * MAX_HISTORY


# ---- refusals, each with its text; the ABI -----------------------------------------------------------------------------------------------------------------------
def check_refusals(L=None):
    assert fh.constants(None, L) == (capi.PT_ERR_INVALID, "null parameters")
    for mf in (1.0, 4.0, 6.0, 3.0e38):
        for k in (0.0, 2.0, 1.0e6):
            for radius in (1, 2, 3):
                assert fh.constants(fh.params(mf, k, radius), L) == (capi.PT_OK, "")
    for mf in (0.0, 0.999, -4.0, np.nan, np.inf, -np.inf):
        assert fh.constants(fh.params(mf, 2.0, 2), L) == (capi.PT_ERR_INVALID, "maxFast must be at least 1 and finite")
    for k in (-1e-30, -2.0, np.nan, np.inf, -np.inf):
        assert fh.constants(fh.params(4.0, k, 2), L) == (capi.PT_ERR_INVALID, "sigmaScale must be non-negative and finite")
    for radius in (0, -1, 4, 2 ** 31 - 1, -2 ** 31):
        assert fh.constants(fh.params(4.0, 2.0, radius), L) == (capi.PT_ERR_INVALID, "radius must be 1, 2 or 3")
    for flags in (1, 2, 1 << 31):
        assert fh.constants(fh.params(4.0, 2.0, 2, flags), L) == (capi.PT_ERR_INVALID, "unknown flag bits")
    assert fh.need_history(True, L) == (capi.PT_OK, "")
    assert fh.need_history(False, L) == (capi.PT_ERR_STATE, "the history was made with pt_temporal_fast off")
    hf, hnf, hc, hn = noisy_planes(5, 4, 1)
    assert fh.clamp(hf, hnf, hc, hn, fh.params(4.0, 2.0, 0), L=L)[0] == capi.PT_ERR_INVALID


def test_refusals_have_their_texts():
    check_refusals()


def test_the_abi_names_the_entries():
    names, debug = [n for n, _, _ in capi.API], [n for n, _, _ in capi.DEBUG_API]
    assert "pt_temporal_fast" in names and "pt_read_temporal_fast" in names and "pt_debug_fast_time" in debug and "pt_debug_fast_time" not in names
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    assert "int pt_temporal_fast(pt_context* ctx, const pt_FastParams* params /* NULL: off */);" in header
    assert "int pt_read_temporal_fast(pt_context* ctx, float* rgba32f_out, float* length_out);" in header
    assert "pt_debug_fast_time" not in header
    from vk_raytrace_amd import host_device as hd
    from vk_raytrace_amd.renderer import HipRenderer
    assert callable(HipRenderer.temporal_fast) and callable(HipRenderer.read_temporal_fast) and isinstance(HipRenderer.fast_params(), hd.FastParams)
    shim = open(os.path.join(ROOT, "include", "pt_renderer.hpp")).read()
    assert "temporalFast(" in shim and "readTemporalFast(" in shim
    for header in ("pt_temporal.h", "pt_svgf.h", "pt_motion.h", "pt_albedo.h", "pt_denoise.h"):     # the parent's operation sequences know nothing of this one
        assert "fast" not in open(os.path.join(fh.CSRC, header)).read().lower().replace("fast math", "").replace("fast-math", "")


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------------------------------------------
def check_hostile_planes_sanitized(header_dir=None):
    """tests/cpp/fast_asan_main.cpp: fast_clamp_pixel over hostile planes in heap blocks of exactly w * h pixels, in a stand-alone program built with
    -fsanitize=address,undefined and run by itself"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fast_asan")
        subprocess.check_call(["g++"] + ([] if header_dir is None else ["-I" + header_dir]) + [c for c in fh.COMPILE if c not in ("-fopenmp", "-fPIC")]
                              + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, ASAN_MAIN])
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 0 and "pixels" in p.stdout, (p.stdout + p.stderr)[-600:]


def test_hostile_planes_sanitized():
    check_hostile_planes_sanitized()


# ---- planted breaks ----------------------------------------------------------------------------------------------------------------------------------------------
FAST_H, UNIT, STEP, COMMON = "pt_fast.h", "fast_host.cpp", "stage/history_step.h", "stage/stage_host_common.h"
BREAKS = {
    "clamp_reads_the_read_set": ([(STEP, "clamp_image(q.out_fast, q.out_fast_length, q.out_colour, q.out_length, q.w, q.h, fk, q.out_colour, q.out_length);",
                                   "clamp_image(q.hist_fast ? q.hist_fast : q.out_fast, q.hist_fast ? q.hist_fast_length : q.out_fast_length, q.out_colour, q.out_length, q.w, q.h, fk, "
                                   "q.out_colour, q.out_length);")],
                                 lambda L: check_step_is_two_steps_then_the_clamp(L)),
    "sigma_without_the_max": ([(FAST_H, "sqrtf(v < 0.0f ? 0.0f : v)", "sqrtf(v)")], lambda L: check_negative_variance_counts_as_zero(L)),
    "length_not_cut": ([(FAST_H, "o.length = k.maxFast < n ? k.maxFast : n;", "o.length = n;")], lambda L: check_length_is_cut_where_a_channel_moved(L)),
    "length_cut_everywhere": ([(FAST_H, "if(o.colour.x != c.x || o.colour.y != c.y || o.colour.z != c.z)", "if(true)")], lambda L: check_length_is_cut_where_a_channel_moved(L)),
    "fast_step_with_max_history": ([(STEP, "kf.maxHistory         = fk.maxFast;", "")], lambda L: check_composition_static((45, 37), "none", False, False, L)),
    "skipped_tap_counted": ([(FAST_H, "      if(!(f.w > 0.0f))\n        continue;  // a tap that does not count is left out of n as well\n      cnt = cnt + 1.0f;",
                              "      cnt = cnt + 1.0f;\n      if(!(f.w > 0.0f))\n        continue;")], lambda L: check_hostile_planes(L)),
    "fast_step_reads_the_raw_colour": ([(STEP, "  step_form(q, kf, q.hist_fast,", "  HistoryCall raw = q;\n  raw.albedo      = nullptr;\n  step_form(raw, kf, q.hist_fast,")],
                                       lambda L: check_composition_static((45, 37), "none", False, True, L)),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_a_planted_break_fails_its_test(name):
    edits, check = BREAKS[name]
    with tempfile.TemporaryDirectory() as tmp:
        os.mkdir(os.path.join(tmp, "stage"))       # the unit's own headers go next to its copy
        for fname, src_dir in ((FAST_H, fh.CSRC), (UNIT, os.path.join(ROOT, "tests", "cpp")), (STEP, os.path.join(ROOT, "tests", "cpp")), (COMMON, os.path.join(ROOT, "tests", "cpp"))):
            text = open(os.path.join(src_dir, fname)).read()
            for _, old, new in [e for e in edits if e[0] == fname]:
                assert text.count(old) == 1, (name, old)
                text = text.replace(old, new)
            open(os.path.join(tmp, fname), "w").write(text)
        out = os.path.join(tmp, "libbroken.so")
        subprocess.check_call(["g++", "-I" + tmp] + fh.COMPILE + ["-shared", "-o", out, os.path.join(tmp, UNIT)])
        L = fh.bind(out)
        with pytest.raises(AssertionError):
            check(L)

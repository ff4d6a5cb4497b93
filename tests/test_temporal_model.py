"""The temporal reprojection stage: the host build of vk_raytrace_amd/csrc/pt_temporal.h (tests/temporal_host.py) against the
float64 model of the definition (tests/golden/gen_temporal_kat.py), its exact properties, and a check of the conventions that shares nothing with the
model's reading of them.  No GPU: tests/test_temporal_gpu.py holds the device to this host build bit for bit.

The bound.  There is no reference leg to measure against, so the tolerance is derived: the model's float64 run carries with every value a running
first-order error bound of an fp32 evaluation of the same operation sequence (gen_temporal_kat.V) -- every operation adds u |result|, u = 2^-24, and one
denormal step to what it inherits; a product inherits |a| e_b + |b| e_a + e_a e_b, a quotient (e_a + |a / b| e_b) / (|b| - e_b), a square root the
difference of the roots of the interval's ends.  The sensitivities of the definition fall out of these rules and are not added by hand: fx and fy
inherit the error of clip.xy divided by clip.w (the quotient rule), t_exp inherits the error of P, which grows with the depth (P = org + dir t).
The count behind it, for orientation: about 30 operations to P (|P| u each), 8 to clip, 6 to fx, so fx is good to some tens of u W / clip.w-relative
units; 4 products and 3 additions per sum, one quotient, and the four operations of the mix.  Where fx or fy lies within its own bound of an integer,
host and model may gather different taps; the tap that differs has a weight of at most |dfx| + |dfy|, and the bound carries that weight, over the sum
of weights, times the range of the history over the 3 x 3 neighbourhood.  The bound is applied as it stands, with 2^-20 relative slack for the float64
evaluation's own rounding.  measure_temporal_kat.py records the host build's worst ratio to it in temporal_kat_tol.json: reported, not used.

Kept pixels: the model alone decides (gen_temporal_kat.judge); its caps are conditions (test_the_fixture_meets_its_caps).

Planted breaks (test_a_planted_break_fails_its_test applies each to a scratch copy of the header, never to the tree, and runs the named check):
    fy built from -clip.y                    host_meets_model (yaw)
    a transposed matrix                      host_meets_model (yaw)
    t_exp taken from eye instead of eye_h    host_meets_model (dolly)
    the depth test dropped                   no_leak_across_a_depth_step
    Hn not advanced                          static_lengths
    weights wx and 1 - wx swapped            host_meets_model (strafe)
    the range guard after the int conversion no_unchecked_conversion: a stand-alone program built with -fsanitize=float-cast-overflow (the results
                                             are the same on x86, where the conversion of a NaN happens to give INT_MIN; only the sanitizer sees it)
    read and write sets not swapped          lives in pt_temporal.hip, not in the header: tests/test_temporal_gpu.py's three-call sequence fails on it
"""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import temporal_host as th
from vk_raytrace_amd import capi, host_device as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_temporal_kat", os.path.join(ROOT, "tests", "golden", "gen_temporal_kat.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

SLACK = 1.0 + 2.0 ** -20
CASES = [(size, move) for size in gen.SIZES for move in gen.MOVES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def history_of(inp):
    H = inp["hist"]
    return None if H is None else th.History(H["colour"], H["guide"], H["length"], H["worldToClip"], H["eye"])


def params_of(inp, max_history=None):
    return th.params(inp["worldToClip"], float(inp["depthTol"]), float(inp["normalDist2"]), float(inp["maxHistory"] if max_history is None else max_history))


def run_host(inp, L=None, hist="own"):
    hist = history_of(inp) if isinstance(hist, str) else hist
    rc, new = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), hist, L=L)
    assert rc == 0
    return new, th.probe(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), hist, L=L)


_judged = {}


def judged(size, move):
    """the model's verdict on a case, computed once and shared"""
    if (size, move) not in _judged:
        inp = gen.case_inputs(size, move)
        _judged[size, move] = (inp, gen.judge(inp))
    return _judged[size, move]


def ratios(inp, r, new, pr):
    """worst error / bound of the host build over the kept pixels: out.rgb, Hn', fx and fy; and whether the outcome classes agree there"""
    n = inp["w"] * inp["h"]
    k = r["kept"]
    out, length, fxfy = new.colour.reshape(n, 4)[:, :3].astype(np.float64), new.length.reshape(n).astype(np.float64), pr["fxfy"].reshape(n, 2).astype(np.float64)
    worst = {}
    with np.errstate(all="ignore"):
        fin = k & (r["outcome"] != gen.NOTHING) & ((r["outcome"] != gen.CURRENT))
        err = np.abs(out - r["out"])
        worst["out"] = float(np.max(np.where(fin[:, None], err / (r["out_e"] * SLACK + 1e-300), 0.0), initial=0.0))
        worst["length"] = float(np.max(np.where(fin, np.abs(length - r["length"]) / (r["length_e"] * SLACK + 1e-300), 0.0), initial=0.0))
        at = k & r["reached"]
        worst["fx"] = float(np.max(np.where(at, np.abs(fxfy[:, 0] - r["fx"]) / (r["fx_e"] * SLACK), 0.0), initial=0.0))
        worst["fy"] = float(np.max(np.where(at, np.abs(fxfy[:, 1] - r["fy"]) / (r["fy_e"] * SLACK), 0.0), initial=0.0))
    # without history the result is the input, bit for bit, and the length exactly 1 or 0
    plain = k & (r["outcome"] >= gen.CURRENT)
    exact = np.array_equal(bits(new.colour.reshape(n, 4)[plain]), bits(inp["colour"].reshape(n, 4)[plain])) and np.array_equal(length[plain], r["length"][plain])
    return worst, bool((pr["outcome"].reshape(n)[k] == r["outcome"][k]).all()), exact


def check_host_meets_model(size, move, L=None):
    inp, r = judged(size, move)
    new, pr = run_host(inp, L)
    worst, classes, exact = ratios(inp, r, new, pr)
    assert classes, f"{size} {move}: outcome classes differ on kept pixels"
    assert exact, f"{size} {move}: a pixel without history is not the current pixel bit for bit"
    assert all(v <= 1.0 for v in worst.values()), f"{size} {move}: error / bound {worst}"
    n = inp["w"] * inp["h"]
    assert np.array_equal(bits(new.colour[..., 3]), bits(inp["colour"][..., 3]))                     # alpha is the current pixel's
    assert np.array_equal(bits(new.guide[..., :3]), bits(inp["g1"][..., :3])) and np.array_equal(bits(new.guide[..., 3]), bits(inp["g2"][..., 0]))
    return worst


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_generator_mints():
    kat = np.load(gen.PATH)
    for move in gen.MOVES:
        _, r = judged(gen.STORED, move)
        assert np.array_equal(kat[f"{move}_out"], r["out"], equal_nan=True) and np.array_equal(kat[f"{move}_length"], r["length"])
        assert np.array_equal(kat[f"{move}_kept"], r["kept"]) and np.array_equal(kat[f"{move}_outcome"], r["outcome"])
        assert np.array_equal(kat[f"{move}_fxfy"], np.stack([r["fx"], r["fy"]], 1), equal_nan=True)


def test_the_fixture_meets_its_caps():
    """at most 5 % of a case dropped, every outcome class kept 50 times, a fifth of the pixels disoccluded by the large move, nothing behind the camera kept"""
    results = {f"{s} {m}": judged(s, m)[1] for s, m in CASES}
    assert (gen.check_caps(results) >= gen.CLASS_FLOOR).all()
    for size in gen.SIZES:
        assert (judged(size, "disocclude")[1]["outcome"] >= gen.CURRENT).mean() >= 0.2
        assert (judged(size, "turn")[1]["outcome"] >= gen.CURRENT).all()
        # the static case keeps its pixels although fx sits on an integer everywhere
        r = judged(size, "none")[1]
        assert r["near_int"].mean() > 0.9 and r["kept"].mean() >= 0.95


# ---- host build against model --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,move", CASES, ids=[f"{s[0]}x{s[1]}-{m}" for s, m in CASES])
def test_host_meets_model(size, move):
    check_host_meets_model(size, move)


def sequence(size, L=None, max_history=3.5):
    """three calls (start, sub-pixel strafe, yaw): call k reads the host build's own output of call k - 1, in the model too, so that errors do not compound.
    Yields (inputs, judged model, host history, host probe) per call."""
    hist = None
    for k, move in enumerate(("first", "strafe", "yaw")):
        inp = gen.case_inputs(size, move)
        inp["maxHistory"] = np.float32(max_history)
        if hist is not None:
            inp["hist"] = {"colour": hist.colour, "guide": hist.guide, "length": hist.length, "worldToClip": hist.world_to_clip, "eye": hist.eye}
        r = gen.judge(inp)
        new, pr = run_host(inp, L, hist=hist)
        yield inp, r, new, pr
        hist = new


def test_a_three_call_sequence_meets_the_model():
    kept = 0
    for k, (inp, r, new, pr) in enumerate(sequence((45, 37))):
        worst, classes, exact = ratios(inp, r, new, pr)
        assert classes and exact and all(v <= 1.0 for v in worst.values()), f"call {k}: {worst}"
        assert 1 - r["kept"].mean() <= gen.DROP_CAP
        kept += int(r["kept"].sum())
    assert kept > 3 * 0.95 * 45 * 37


# ---- exact properties ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_first_call_returns_the_current_image():
    inp = gen.case_inputs((45, 37), "first")
    new, pr = run_host(inp)
    assert np.array_equal(bits(new.colour), bits(inp["colour"]))
    assert np.array_equal(new.length, np.where(gen.finite3(inp["colour"]), 1.0, 0.0).astype(np.float32))
    assert (pr["verdicts"] == 0).all()


def check_static_lengths(L=None):
    """with a static camera the lengths of three calls are 2, 3, min(4, maxHistory) within the bound, where the current pixels were finite throughout"""
    for max_history in (8.0, 3.5):
        inp = gen.case_inputs((45, 37), "first")
        inp["maxHistory"] = np.float32(max_history)
        fin = gen.finite3(inp["colour"])
        rc, hist = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), None, L=L)
        assert rc == 0
        for want in (2.0, 3.0, min(4.0, max_history)):
            inp["colour"] = gen.noisy_colour(45, 37, np.random.default_rng(int(want * 10)))
            inp["hist"] = {"colour": hist.colour, "guide": hist.guide, "length": hist.length, "worldToClip": hist.world_to_clip, "eye": hist.eye}
            r = gen.judge(inp)
            rc, hist = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], params_of(inp), history_of(inp), L=L)
            assert rc == 0
            fin &= gen.finite3(inp["colour"])
            sel = fin.reshape(-1) & r["kept"] & (r["outcome"] == gen.BLEND)
            assert sel.sum() > 0.8 * 45 * 37
            assert (np.abs(hist.length.reshape(-1)[sel] - want) <= r["length_e"][sel] * SLACK).all(), want
            assert (np.abs(r["length"][sel] - want) <= r["length_e"][sel] * SLACK).all()


def test_static_lengths():
    check_static_lengths()


def check_no_leak(L=None):
    """A tap across a depth step of many tolerances cannot influence the output: overwrite the colours of every history pixel that some output pixel
    looks at across such a step with other values, Inf included, and no bit moves in any output pixel that sees the overwritten pixels only across the
    step (the silhouettes of the box against wall and floor after the yaw).  The denoiser's leak test."""
    w, h = 96, 64
    inp = gen.case_inputs((w, h), "yaw")
    n = w * h
    new, pr = run_host(inp, L)
    H = inp["hist"]
    t_exp = pr["point"].reshape(n, 4)[:, 3]
    taps, verdicts = pr["taps"].reshape(n, 4, 2), pr["verdicts"].reshape(n, 4)
    hg = H["guide"].reshape(n, 4)
    inside = (verdicts != 0) & (verdicts != th.OUTSIDE)
    at = np.where(inside, taps[..., 1] * w + taps[..., 0], 0)
    with np.errstate(invalid="ignore"):
        far = inside & (np.abs(hg[at, 3] - t_exp[:, None]) > 5 * gen.DEPTH_TOL * t_exp[:, None])   # off by more than five tolerances
    overwritten = np.zeros(n, bool)
    overwritten[at[far]] = True
    untouched = ~(inside & ~far & overwritten[at]).any(1)   # output pixels that see overwritten history only across the step, if at all
    witnesses = untouched & far.any(1)
    assert witnesses.sum() >= 20, int(witnesses.sum())
    for value in (1.0e6, np.inf, -7.0):
        hc = H["colour"].copy().reshape(n, 4)
        hc[overwritten, :3] = value
        again, _ = run_host(dict(inp, hist=dict(H, colour=hc.reshape(h, w, 4))), L)
        same = (bits(again.colour.reshape(n, 4)) == bits(new.colour.reshape(n, 4))).all(1) & (bits(again.length.reshape(n)) == bits(new.length.reshape(n)))
        assert same[untouched].all(), (value, int((~same[untouched]).sum()))


def test_no_leak_across_a_depth_step():
    check_no_leak()


def test_a_non_finite_current_pixel_returns_the_history_and_keeps_its_length():
    inp = gen.case_inputs((45, 37), "none")
    n = 45 * 37
    H = inp["hist"]
    inp["colour"][..., :3] = np.nan     # every pixel: the output is then the gathered history alone
    new, pr = run_host(inp)
    have = pr["outcome"].reshape(n) == th.HISTORY_ONLY
    assert have.sum() > 0.9 * n and ((pr["outcome"].reshape(n) == th.NOTHING) | have).all()
    # static camera: the tap of weight 1 (or within rounding of it) is the pixel itself
    r = gen.judge(inp)
    k = r["kept"] & have
    assert (np.abs(new.colour.reshape(n, 4)[k, :3] - H["colour"].reshape(n, 4)[k, :3]) <= r["out_e"][k] * SLACK).all()
    assert (np.abs(new.length.reshape(n)[k] - H["length"].reshape(n)[k]) <= r["length_e"][k] * SLACK).all()
    assert (new.length.reshape(n)[~have] == 0).all()


def test_a_pixel_of_length_zero_is_never_gathered():
    inp = gen.case_inputs((45, 37), "yaw")
    H = inp["hist"]
    n = 45 * 37
    new, pr = run_host(inp)
    dead = H["length"].reshape(n) < 1
    assert dead.sum() > 10
    taps, verdicts = pr["taps"].reshape(n, 4, 2), pr["verdicts"].reshape(n, 4)
    counted = verdicts == th.COUNTED
    at = np.where(counted, taps[..., 1] * 45 + taps[..., 0], 0)
    assert not (counted & dead[at]).any()
    # ... whatever they hold: finite colours there change nothing
    hc = H["colour"].copy().reshape(n, 4)
    hc[dead, :3] = 123.0
    other = dict(inp, hist=dict(H, colour=hc.reshape(37, 45, 4)))
    again, _ = run_host(other)
    assert np.array_equal(bits(again.colour), bits(new.colour)) and np.array_equal(bits(again.length), bits(new.length))


SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1.0e-45, -1.0e-45, 1.0e-39, 1.0, -1.0, 0.5, 1.0e18, 1.0e19, 7.0e9], np.float32)


def adversarial(rng, w, h):
    """one call's worth of hostile inputs: a history camera of special values and random bit patterns, depths likewise, clip.w of +-0 among them"""
    def words(k):
        v = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32).view(np.float32)
        pick = rng.uniform(size=k) < 0.5
        return np.where(pick, rng.choice(SPECIAL, k), v).astype(np.float32)
    inp = gen.case_inputs((w, h), "yaw")
    H = dict(inp["hist"])
    H["worldToClip"] = words(16)
    if rng.uniform() < 0.3:
        H["worldToClip"][[3, 7, 11, 15]] = rng.choice(np.array([0.0, -0.0], np.float32), 4)    # clip.w = +-0
    H["eye"] = words(3)
    g2 = inp["g2"].copy()
    g2[..., 0] = words(w * h).reshape(h, w)
    if rng.uniform() < 0.5:
        inp["viewInverse"] = np.where(rng.uniform(size=16) < 0.2, words(16), inp["viewInverse"]).astype(np.float32)
    return dict(inp, g2=g2, hist=H)


def test_no_index_leaves_the_image():
    """adversarial worldToClip matrices and depths: zero, NaN, +-Inf, 3e38, denormals, clip.w of +-0, random bit patterns -- every tap the pixel looks at
    is next to the image at worst, and every tap it counts lies inside"""
    rng = np.random.default_rng(5)
    w, h = 13, 9
    patterns = 0
    for _ in range(100):
        inp = adversarial(rng, w, h)
        _, pr = run_host(inp)
        v, t = pr["verdicts"], pr["taps"]
        seen = v != 0
        assert (t[..., 0][seen] >= -1).all() and (t[..., 0][seen] <= w).all() and (t[..., 1][seen] >= -1).all() and (t[..., 1][seen] <= h).all()
        inside = seen & (v != th.OUTSIDE)
        assert (t[..., 0][inside] >= 0).all() and (t[..., 0][inside] < w).all() and (t[..., 1][inside] >= 0).all() and (t[..., 1][inside] < h).all()
        patterns += w * h
    assert patterns >= 10 ** 4


CAST_MAIN = os.path.join(ROOT, "tests", "cpp", "temporal_cast_main.cpp")


def check_no_unchecked_conversion(header_dir=None):
    """tests/cpp/temporal_cast_main.cpp: temporal_pixel over hostile inputs in a stand-alone program built with -fsanitize=float-cast-overflow -- a float
    that reaches a conversion to int without having passed the range tests ends it"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "temporal_cast")
        subprocess.check_call(["g++"] + ([] if header_dir is None else ["-I" + header_dir]) + [c for c in th.COMPILE if c not in ("-fopenmp", "-fPIC")]
                              + ["-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe, CAST_MAIN])
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 0 and "pixels" in p.stdout, p.stderr[-400:]


def test_no_unchecked_conversion():
    check_no_unchecked_conversion()


def test_temporal_constants_refuses_with_its_own_reason():
    good = dict(depth_tol=0.02, normal_dist2=0.02, max_history=8.0)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    assert th.constants(th.params(eye, **good)) == (0, "")
    assert th.constants(th.params(eye, 1e-30, 0.0, 1.0)) == (0, "")
    reasons = set()
    bad = eye.copy()
    bad[7] = np.nan
    cases = [(None, "null")] + [(th.params(m, **good), "worldToClip") for m in (bad, np.where(eye > 0, np.inf, 0).astype(np.float32))]
    cases += [(th.params(eye, **dict(good, depth_tol=v)), "depthTol") for v in (0.0, -1.0, np.nan, np.inf)]
    cases += [(th.params(eye, **dict(good, normal_dist2=v)), "normalDist2") for v in (-1e-9, np.nan, np.inf)]
    cases += [(th.params(eye, **dict(good, max_history=v)), "maxHistory") for v in (0.99, 0.0, np.nan, np.inf)]
    cases += [(th.params(eye, flags=f, **good), "flag") for f in (1, 0x80000000)]
    for p, word in cases:
        rc, why = th.constants(p)
        assert rc == capi.PT_ERR_INVALID and word in why, (word, why)
        reasons.add(why)
    assert len(reasons) == 6


# ---- conventions, from outside --------------------------------------------------------------------------------------------------------------------------------
def lookat_cameras(cam, aspect):
    """pt_camera_lookat's inverses and pt_camera_world_to_clip's forward matrix for a camera of the generator (eye, center; up = y; the generator's fov)"""
    L = capi.lib()
    out, w2c = hd.SceneCamera(), np.zeros(16, np.float32)
    e, c, u = np.asarray(cam["eye"], np.float32), np.asarray(cam["center"], np.float32), np.array([0, 1, 0], np.float32)
    assert L.pt_camera_lookat(e.ctypes.data, c.ctypes.data, u.ctypes.data, gen.FOV, aspect, C.byref(out)) == 0
    assert L.pt_camera_world_to_clip(e.ctypes.data, c.ctypes.data, u.ctypes.data, gen.FOV, aspect, w2c.ctypes.data) == 0
    return np.array(out.viewInverse, np.float32), np.array(out.projInverse, np.float32), w2c


def previous_camera_ray(vi32, pi32, x, y, w, h):
    """the ray of a camera through the continuous pixel position (x, y), as gen_path_kat.render_frame builds it in float64 (its lines for ux .. direction)"""
    vi, pi = vi32.astype(np.float64).reshape(4, 4).T, pi32.astype(np.float64).reshape(4, 4).T
    ux, uy = x / w, y / h
    dx, dy = ux * 2 - 1, uy * 2 - 1
    tgt = np.stack([pi[r, 0] * dx + pi[r, 1] * dy + pi[r, 2] + pi[r, 3] for r in range(3)], 1)
    tgt /= np.linalg.norm(tgt, axis=1)[:, None]
    d = tgt @ vi[:3, :3].T
    return vi[:3, 3], d / np.linalg.norm(d, axis=1)[:, None]


def convention_residual(size, move, source="host"):
    """max over the pixels with history of |eye_h + ray_h(fx + 0.5, fy + 0.5) |P - eye_h| - P| / |P - eye_h|.  source: the host build's probe, or the
    model's float32 / float64 run"""
    w, h = size
    inp = gen.case_inputs(size, move)
    cur, prev = lookat_cameras(inp, w / h), lookat_cameras({"eye": inp["hist"]["eye64"], "center": inp["hist"]["center64"]}, w / h)
    inp.update(viewInverse=cur[0], projInverse=cur[1], worldToClip=cur[2])
    inp["hist"].update(worldToClip=prev[2], eye=prev[0][12:15].copy())
    n = w * h
    if source == "host":
        _, pr = run_host(inp)
        fx, fy, P = pr["fxfy"].reshape(n, 2)[:, 0], pr["fxfy"].reshape(n, 2)[:, 1], pr["point"].reshape(n, 4)[:, :3]
        have = pr["outcome"].reshape(n) <= th.HISTORY_ONLY
    else:
        r = gen.evaluate(inp, np.float32 if source == "f32" else np.float64)
        fx, fy, P, have = r["fx"], r["fy"], r["point"], r["outcome"] <= gen.HISTORY_ONLY
    assert have.sum() > 0.3 * n
    fx, fy, P = fx[have].astype(np.float64), fy[have].astype(np.float64), P[have].astype(np.float64)
    o, d = previous_camera_ray(prev[0], prev[1], fx + 0.5, fy + 0.5, w, h)
    dist = np.linalg.norm(P - o, axis=1)
    return float((np.linalg.norm(o + d * dist[:, None] - P, axis=1) / dist).max())


CONVENTION_MOVES = ("none", "strafe", "yaw", "dolly", "disocclude")


def identity_defect(size):
    """worldToClip (viewInverse projInverse) against the identity over the cameras of the moves, from the fp32 words of pt_camera_world_to_clip and
    pt_camera_lookat, evaluated in float64: (largest |X - 1| relative to |worldToClip| |viewInverse| |projInverse|, the size of the terms each entry sums;
    largest |X - 1| as it stands; largest |worldToClip - proj view| against the generator's own float64 lookat)"""
    scaled = absolute = helper = 0.0
    for move in gen.MOVES:
        inp = gen.case_inputs(size, move)
        vi, pi, w2c = (m.astype(np.float64).reshape(4, 4).T for m in lookat_cameras(inp, size[0] / size[1]))
        defect = np.abs(w2c @ (vi @ pi) - np.eye(4))
        scaled = max(scaled, float((defect / (np.abs(w2c) @ (np.abs(vi) @ np.abs(pi)))).max()))
        absolute = max(absolute, float(defect.max()))
        view, proj = gen.lookat(inp["eye"].astype(np.float32).astype(np.float64), inp["center"].astype(np.float32).astype(np.float64), size[0] / size[1])
        helper = max(helper, float(np.abs(proj @ view - w2c).max()))
    return scaled, absolute, helper


@pytest.mark.parametrize("move", CONVENTION_MOVES)
def test_conventions_through_the_previous_camera(move):
    """y-flip, column-major order, forward against inverse: where the host build says the history camera saw P, that camera's own ray -- built from
    pt_camera_lookat's inverses, not from the forward matrix the stage used -- must pass through P.  Tolerance: 4 x the spread the model's float32 and
    float64 runs show on the same quantity, as recorded in temporal_kat_tol.json."""
    tol = json.load(open(gen.TOL_PATH))["convention_spread"][move]
    got = convention_residual((96, 64), move)
    assert got <= 4 * tol, (got, tol)


def test_world_to_clip_inverts_the_lookat_inverses():
    """worldToClip (viewInverse projInverse) is the identity within 1e-6 of the size of the terms each entry sums, and pt_camera_world_to_clip is within 1e-6 of
    the generator's float64 proj view.  As it stands, without the scale, |X - 1| reaches 3.3e-4 in the two columns that projInverse's entries of
    1 / near = 1000 feed: 1000 x 2^-24 = 6e-5 per term is the precision of the fp32 words pt_camera_lookat returns, not an error of either helper (columns
    0 and 1, which see no such entry, are within 1e-7 unscaled).  temporal_kat_tol.json records all three figures."""
    scaled, absolute, helper = identity_defect((96, 64))
    assert scaled <= 1e-6 and helper <= 1e-6, (scaled, absolute, helper)


# ---- planted breaks -------------------------------------------------------------------------------------------------------------------------------------------
BREAKS = {
    "fy_negated": (("(cly / clw)", "(-cly / clw)"), lambda L, d: check_host_meets_model((96, 64), "yaw", L)),
    "transposed": (("return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w;", "return ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] * w;"),
                   lambda L, d: check_host_meets_model((96, 64), "yaw", L)),
    "t_exp_from_eye": (("Px - k.eyeH[0], ey = Py - k.eyeH[1], ez = Pz - k.eyeH[2]", "Px - ox, ey = Py - oy, ez = Pz - oz"), lambda L, d: check_host_meets_model((96, 64), "dolly", L)),
    "depth_test_dropped": (("else if(!(ptf_abs(hq.w - tExp) <= k.depthTol * tExp))", "else if(false)"), lambda L, d: check_no_leak(L)),
    "length_not_advanced": (("const float n1 = N + 1.0f;", "const float n1 = N;"), lambda L, d: check_static_lengths(L)),
    "weights_swapped": (("const float wx = fx - x0f,", "const float wx = 1.0f - (fx - x0f),"), lambda L, d: check_host_meets_model((96, 64), "strafe", L)),
    "guard_after_conversion": (("if(fx > -1.0f && fx < float(w) && fy > -1.0f && fy < float(h))", "if(int(floorf(fx)) >= -1 && int(floorf(fx)) < w && int(floorf(fy)) >= -1 && int(floorf(fy)) < h)"),
                               lambda L, d: check_no_unchecked_conversion(d)),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_a_planted_break_fails_its_test(name):
    (old, new), check = BREAKS[name]
    text = open(os.path.join(th.CSRC, "pt_temporal.h")).read()
    assert text.count(old) == 1, name
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "pt_temporal.h"), "w").write(text.replace(old, new))
        L = None if name == "guard_after_conversion" else th.bind(th.compile_to(os.path.join(tmp, "libbroken.so"), header_dir=tmp))
        with pytest.raises((AssertionError, subprocess.CalledProcessError)):
            check(L, tmp)

"""The denoiser's host build (vk_raytrace_amd/csrc/pt_denoise.h compiled by g++: tests/denoise_host.py) against the float64 model of
tests/golden/gen_denoise_kat.py, which is written from the definition (DESIGN.md "Denoiser") and shares no code with the header.  The device is held bit
for bit to the host build by tests/test_denoise_gpu.py, so this is where the arithmetic is judged.

Per iteration.  The model is fed the host build's fp32 output of iteration i - 1 (for iteration 0 the input, demodulated in np.float32 -- one IEEE division
per channel, reproducible bit for bit), so errors do not compound, and every judged pixel must lie within the bound derived here.

The bound (u = 2^-24, the unit roundoff; all of it is evaluated per pixel and channel by gen_denoise_kat.iteration from the float64 quantities):
  exponent   e = sum of at most 4 non-negative terms d * inv.  A distance d = dx^2 + dy^2 + dz^2 takes 4 roundings on non-negative summands (difference,
             square, two additions), the product with the fp32 constant inv one more, the additions of the terms at most 3: e_fp32 = e (1 + t), |t| <=
             (1 + u)^8 - 1.  Operations whose result is denormal add at most 2^-149 each, scaled by the largest constant: 8 * 2^-149 * max(inv) absolutely.
  exp        exp(-e_fp32) = exp(-e) exp(-e t): the exponent's error is AMPLIFIED BY |e|, relative change rho = expm1(e ((1 + u)^8 - 1) + 8 * 2^-149 max(inv)).
             pt_exp itself is held to 1.1 ulp by tests/test_fpmath.py: relative 1.1 * 2 u in the normal range (1 ulp <= 2 u |x|), and absolutely 1.1 * 2^-149
             where the result is denormal; below the range that test samples (arguments under -103) the true value is under 1.4 * 2^-149 and pt_exp returns
             0 or 2^-149, so 2 * 2^-149 covers the whole denormal and flushed range.
  weight     w = k exp(-e) with k = h h exact (products of 1/16, 1/4, 3/8): one rounding.  w_fp32 = w (1 + delta) + eta with
             1 + delta <= (1 + rho)(1 + 2.2 u)(1 + u) and eta = k * 2 * 2^-149 + 2^-149.
  sums       at most 25 products w c (one rounding each, 2^-149 if denormal) added in tap order: a term passes through at most 24 additions, so
             |num_fp32 - num| <= sum |w c| ((1 + delta)(1 + u)^25 - 1) + sum (eta |c| + 2^-149)(1 + u)^25 =: dN, and for the weights alone
             |den_fp32 - den| <= sum w ((1 + delta)(1 + u)^24 - 1) + sum eta (1 + u)^24 =: dD.
  division   |num_fp32 / den_fp32 - num / den| <= (dN + |num / den| dD) / (den - dD), then one rounding: times (1 + u), plus u |num / den|, plus 2^-149.
             den - dD > den / 2 is asserted for every judged pixel (a finite centre contributes its own weight 9/64, e = 0).
  model      the float64 evaluation's own error (2^-53 per operation over the same operation count) is covered by a relative allowance of 2^-20 on the bound.
The constants are recorded in tests/golden/denoise_kat_tol.json with the worst ratio of the host build's error to this bound that
`gen_denoise_kat.py --measure` observed (0.17: a worst-case bound over 25 taps sits well above what rounding errors of mixed sign add up to); the test
asserts ratio <= 1 and does not read the observed figure.

Pixels the model does not judge: centre colour not finite and 0 < float64 sum of weights < 1e-30 (the underflow of the fp32 exp decides between a mean and the
unchanged pixel); at most 1 % of the pixels of any iteration of any case.  A float64 sum of exactly 0 is judged exactly: the pixel comes back unchanged.

Exact properties (no tolerance): edge isolation, non-finite repair, the isolated non-finite pixel, alpha; the pure linear filter within the bound above.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from tests import denoise_host as dh
from vk_raytrace_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_denoise_kat", os.path.join(ROOT, "tests", "golden", "gen_denoise_kat.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_kat = None


def kat():
    global _kat
    if _kat is None:
        _kat = gen.load()
    return _kat


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def judge_call(colour, guides, iterations, sigma_color, sigma_guide, flags, what):
    """One call of the host build, every iteration held to the model.  Returns (worst ratio error / bound, largest left-out fraction)."""
    p = dh.params(iterations, sigma_color, sigma_guide, flags)
    rc, out, its = dh.denoise(colour, guides, p, per_iteration=True)
    assert rc == 0, what
    inv_c, inv_g = gen.constants(sigma_color, sigma_guide)
    planes = sum(1 << j for j in range(3) if guides[j] is not None)
    rc, h_inv_c, h_inv_g, terms = dh.constants(p, planes)
    assert rc == 0 and terms == (1 if sigma_color > 0 else 0) | planes << 1, what
    assert np.array_equal(bits(h_inv_c[:iterations]), bits(inv_c[:iterations])), what  # fp32 by definition
    assert all(h_inv_g[j] == inv_g[j] for j in range(3) if guides[j] is not None), what
    cur = gen.demodulate(colour, guides[0]) if flags & gen.DEMODULATE else np.ascontiguousarray(colour, np.float32)
    worst, worst_left = 0.0, 0.0
    for i in range(iterations):
        r = gen.iteration(cur, guides, i, inv_c[i], inv_g, sigma_color > 0)
        got = its[i]
        tag = f"{what} iteration {i}"
        assert np.array_equal(bits(got[..., 3]), bits(cur[..., 3])), f"{tag}: alpha is not the centre's"
        same = r["unchanged"]
        assert np.array_equal(bits(got[..., :3])[same], bits(cur[..., :3])[same]), f"{tag}: a pixel without weights did not come back unchanged"
        left = r["left_out"]
        worst_left = max(worst_left, float(left.mean()))
        assert left.mean() <= gen.LEFT_OUT_CAP, f"{tag}: {left.sum()} pixels left out"
        judged = ~same & ~left
        g = got[..., :3].astype(np.float64)[judged]
        assert np.isfinite(g).all(), f"{tag}: a judged pixel is not finite"
        err, bound = np.abs(g - r["rgb"][judged]), r["bound"][judged]
        ratio = float((err / bound).max()) if err.size else 0.0
        print(f"{tag}: judged {int(judged.sum())}, unchanged {int(same.sum())}, left out {int(left.sum())}, worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, f"{tag}: error {ratio:.3f} x the bound"
        worst = max(worst, ratio)
        cur = got
    want = gen.remodulate(its[-1], guides[0]) if flags & gen.DEMODULATE else its[-1]
    assert np.array_equal(bits(out), bits(want)), f"{what}: the result is not the last iteration{' times the albedo' if flags else ''}"
    return worst, worst_left


def judge_size(w, h, iterations):
    colour, guides = gen.inputs(kat(), w, h)
    worst = 0.0
    for col, installed, flags in gen.cases():
        r, _ = judge_call(colour, gen.case_guides(guides, installed), iterations, gen.SIGMA_COLOR if col else 0.0, gen.SIGMA_GUIDE, flags,
                          f"{w}x{h} x{iterations} colour={int(col)} guides={''.join(str(int(b)) for b in installed)} flags={flags}")
        worst = max(worst, r)
    return worst


def worst_ratio_over_fixture():
    """what gen_denoise_kat.py --measure records"""
    return max([judge_size(w, h, n) for w, h in gen.SIZES + ((1, 1),) for n in gen.ITERATIONS])


@pytest.mark.parametrize("iterations", gen.ITERATIONS)
@pytest.mark.parametrize("size", gen.SIZES + ((1, 1),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_build_meets_the_model_per_iteration(size, iterations):
    """every on / off combination of the colour term, each guide and the demodulation; 8 iterations reach step 128, beyond both images"""
    judge_size(size[0], size[1], iterations)


def test_fixture_is_what_the_generator_builds_and_keeps_its_cap():
    fresh = gen.build()
    assert sorted(fresh) == sorted(kat())
    for k in fresh:
        assert np.asarray(fresh[k]).dtype == kat()[k].dtype and np.asarray(fresh[k]).tobytes() == kat()[k].tobytes(), k
    assert os.path.getsize(gen.PATH) < 400 * 1024
    w, h = gen.SIZES[1]
    colour, guides = gen.inputs(kat(), w, h)
    assert (~gen.finite3(colour)).sum() >= 9
    for col, installed, flags in gen.cases()[::5]:   # the generator asserts the cap on every case when it writes the fixture; a sample here
        for i, _, r in gen.chain(colour, gen.case_guides(guides, installed), 5, gen.SIGMA_COLOR if col else 0.0, gen.SIGMA_GUIDE, flags):
            assert r["left_out"].mean() <= gen.LEFT_OUT_CAP


def step_scene(w=40, h=24, x_edge=17, seed=3):
    rng = np.random.default_rng(seed)
    colour = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 4))).astype(np.float32)
    guide = np.zeros((h, w, 4), np.float32)
    guide[:, x_edge:, 0] = 1.0
    return colour, guide


def test_edge_isolation_is_exact():
    """a guide step of 1.0 under sigmaGuide = 0.01 (e >= 1e4: the weight is 0): what lies across the edge cannot reach this side, bit for bit"""
    a, guide = step_scene()
    b = a.copy()
    b[:, 17:, :3] = np.exp(np.random.default_rng(4).uniform(np.log(1e-3), np.log(1e3), b[:, 17:, :3].shape)).astype(np.float32)
    for sigma_color in (0.0, 2.0):
        p = dh.params(5, sigma_color, (1.0, 0.01, 1.0))
        _, oa = dh.denoise(a, [None, guide, None], p)
        _, ob = dh.denoise(b, [None, guide, None], p)
        assert np.array_equal(bits(oa[:, :17]), bits(ob[:, :17]))
        assert not np.array_equal(bits(oa[:, 17:]), bits(ob[:, 17:]))


def test_non_finite_pixels_are_repaired_by_finite_neighbours():
    """NaN and +-Inf pixels, each with a finite pixel in its 5 x 5 step-1 neighbourhood and equal guides: finite everywhere after iteration 0"""
    rng = np.random.default_rng(5)
    colour = rng.uniform(0.1, 10.0, (20, 31, 4)).astype(np.float32)
    guide = np.full((20, 31, 4), 0.5, np.float32)
    colour[3, 3, :3] = np.nan
    colour[3, 4, 0] = np.inf
    colour[4, 3, 1] = -np.inf
    colour[0, 0, :3] = (np.nan, np.inf, -np.inf)
    colour[19, 30, 2] = np.nan
    colour[10:14, 10:14, :3] = np.nan   # a 4 x 4 block: every pixel of it still has a finite one within two steps
    for sigma_color in (0.0, 1.0):
        for guides in ([None, None, None], [guide, guide, None]):
            _, out, its = dh.denoise(colour, guides, dh.params(2, sigma_color, (0.1, 0.1, 0.1)), per_iteration=True)
            assert np.isfinite(its[0]).all() and np.isfinite(out).all()


def test_isolated_non_finite_pixel_comes_back_unchanged():
    """a non-finite pixel whose guide differs by 1.0 from every neighbour (sigmaGuide 0.01): no tap has a weight, the pixel returns bit for bit -- and it
    does not leak: its neighbours equal those of an image where it is finite"""
    rng = np.random.default_rng(6)
    colour = rng.uniform(0.1, 10.0, (15, 15, 4)).astype(np.float32)
    guide = np.zeros((15, 15, 4), np.float32)
    guide[7, 7, 1] = 1.0
    for v in ((np.nan, 1.0, 2.0), (np.inf, np.inf, np.inf), (1.0, -np.inf, np.nan)):
        c = colour.copy()
        c[7, 7, :3] = v
        for iterations in (1, 4):
            _, out = dh.denoise(c, [None, None, guide], dh.params(iterations, 1.0, (1.0, 1.0, 0.01)))
            assert np.array_equal(bits(out[7, 7]), bits(c[7, 7]))
            _, ref = dh.denoise(colour, [None, None, guide], dh.params(iterations, 1.0, (1.0, 1.0, 0.01)))
            mask = np.ones((15, 15), bool)
            mask[7, 7] = False
            assert np.array_equal(bits(out)[mask], bits(ref)[mask]) and np.isfinite(out[mask]).all()


def test_without_terms_one_iteration_is_the_b3_spline_filter():
    """colour term off, no guides: an interior pixel is sum(k c_q) (the weights sum to 1), within the bound of the docstring"""
    rng = np.random.default_rng(7)
    colour = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (12, 14, 4))).astype(np.float32)
    _, out = dh.denoise(colour, [None, None, None], dh.params(1, 0.0))
    k2 = np.outer(gen.H5, gen.H5)
    c = colour.astype(np.float64)
    r = gen.iteration(colour, [None, None, None], 0, np.float32(0), np.zeros(3, np.float32), False)
    for y in range(2, 10):
        for x in range(2, 12):
            want = (k2[..., None] * c[y - 2:y + 3, x - 2:x + 3, :3]).sum((0, 1))
            assert abs(r["sumw"][y, x] - 1.0) < 1e-15 and np.allclose(want, r["rgb"][y, x], rtol=1e-13)
            assert (np.abs(out[y, x, :3] - want) <= r["bound"][y, x]).all()
    assert np.array_equal(bits(out[..., 3]), bits(colour[..., 3]))


def test_parameter_validation():
    c = np.ones((4, 4, 4), np.float32)
    g = np.ones((4, 4, 4), np.float32)
    INVALID, STATE = capi.PT_ERR_INVALID, capi.PT_ERR_STATE
    run = lambda p, guides=(None, None, None): dh.denoise(c, list(guides), p)[0]
    assert run(dh.params(1, 1.0)) == 0 and run(dh.params(8, 0.0)) == 0
    assert run(dh.params(0, 1.0)) == INVALID and run(dh.params(9, 1.0)) == INVALID and run(dh.params(-1, 1.0)) == INVALID
    assert run(dh.params(1, -1.0)) == INVALID and run(dh.params(1, float("nan"))) == INVALID and run(dh.params(8, 1e-18)) == INVALID
    assert run(dh.params(1, 1.0, flags=2)) == INVALID and run(dh.params(1, 1.0, flags=3), (g, None, None)) == INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30):
        assert run(dh.params(1, 1.0, (1.0, bad, 1.0)), (None, g, None)) == INVALID
        assert run(dh.params(1, 1.0, (1.0, bad, 1.0)), (g, None, g)) == 0          # read only for installed planes
    assert run(dh.params(1, 1.0, flags=gen.DEMODULATE)) == STATE and run(dh.params(1, 1.0, flags=gen.DEMODULATE), (None, g, g)) == STATE
    assert run(dh.params(1, 1.0, flags=gen.DEMODULATE), (g, None, None)) == 0
    # through the C ABI, where no GPU is needed: a null context is an error, not a crash
    L = capi.lib()
    p = dh.params(1, 1.0)
    assert L.pt_denoise(None, C.byref(p), c.ctypes.data) == INVALID
    assert L.pt_tonemap_denoised(None, C.byref(p), None, None) == INVALID
    assert L.pt_set_denoise_guides(None, None) == INVALID
    assert capi.PT_DENOISE_DEMODULATE == gen.DEMODULATE

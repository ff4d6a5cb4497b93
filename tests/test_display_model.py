"""The display pass and its mip chain held to an INDEPENDENT float64 model of the Vulkan rules -- the CPU legs.

test_mip_chain, test_post_frag, test_post_frag_descaling, test_tonemap_matches_oracle and test_post_frag_hip compare one restatement of the Vulkan rules with
another: the vkCmdBlitImage(LINEAR) chain, the NEAREST / NEAREST / REPEAT sampler with its level selection and the float -> UNORM8 store are written out once
in oracle/ref_glue/ (what the compiled post.frag runs on), once in the oracle and once in the kernels.  tests/golden/gen_display_kat.py is the leg that shares
nothing with them (numpy, from the shader text and the specification, float64).  Here the oracle (orc_mip_chain, orc_tonemap_zoom) and the compiled reference
(ref_mip_chain, ref_tonemap) are held to it; tests/test_display_gpu.py holds the device to it and to the oracle.

Bound for a mip level (test_every_mip_level...).  One blit computes, per channel, top = t00 (1 - a) + t10 a, bot likewise, top (1 - b) + bot b in float32.
  * the weights: the legs form u = (x + 0.5) * fl(sw / dw) - 0.5 in float32.  fl(sw / dw) is off by at most 2^-24 relative, (x + 0.5) <= dw, so u is off by at
    most sw 2^-24 from the ratio and as much again from rounding the product (|u| < sw); the subtraction of 0.5 and of floor(u) are exact.  So |a - a_exact| <=
    sw 2^-23, |b - b_exact| <= sh 2^-23 (where a crosses an integer the two texels swap roles and the result is continuous), and the result moves by at most
    (sw + sh) 2^-23 max|texel| (non-negative texels: |t10 - t00| <= max|texel|).
  * the arithmetic: 1 - a, two products and a sum, three times over: fewer than 8 roundings of values <= max|texel|, 8 x 2^-24 = 4 x 2^-23.
  One level therefore adds (sw + sh + 4) 2^-23 max|texel of the source level| -- the form tests/test_texture_model.py uses for a bilinear tap -- and inherits the
  bound of the level below, because the filter is a convex combination.  The fixture stores the model rounded to float32: + 2^-24 |texel|.

fragColor, per case, on kept pixels: within 4 x the error the compiled reference itself shows against the model (tests/golden/display_kat_tol.json, written by
tests/golden/measure_display_kat.py; guard rail 1e-3), in the measure |a - b| / (|b| + 1e-6).  The kept mask is the model's alone (gen_display_kat.py).
Local-exposure exit: the legs return fragColor only, so a leg's exit is recovered from it: the model re-evaluates fragColor for each of the eight exits and the
leg's pixel must be explained best -- and within the bound -- by the exit the model recorded; every exit is observed that way on at least 50 kept pixels whose
other candidates are all further than twice the bound away.
UNORM8 codes, from each leg's floats by the project's store (orc_unorm8): the model's on kept pixels, within 1 on pixels dropped for the final rounding only.
Oracle and compiled reference: bit-identical on every stored pixel, edge runs included.

What this found.  toneLocalExposure (post.frag:82-83) calls texture(inImage, uv, i): the third argument is a LOD bias.  With tm.zoom = 1/2 or 1/3 (the viewer
navigating) lambda_base = log2(zoom) is negative, so the levels read are nearest(max(0, i - 1)) and nearest(max(0, i - 1.585)) -- not i.  ref_driver.h, the oracle
and k_tonemap all read level i ("implicit LOD 0") and agreed with each other bit for bit.  Against the model, on the 37 x 26 render shown in 75 x 53 at zoom 1/2
with autoExposure = 3, 321 of 3906 kept pixels differed by up to 5 codes (fragColor off by 3e-2 where the reference's own error is 8e-8), and the exit test
failed; on the zoom 1/3 run the images happen to coincide (the padded chain's 1 x 1 level is nearly black there, the scaled luminances are in the hundreds, the
key term of the break test vanishes and both readings leave the loop with level 0's value).  All three legs now take the level from log2(zoom) (computed on the
host for the kernel).  At zoom 1 nothing changes, so no stored golden image moved.
The store floor(clamp(v) * 255 + 0.5) handed a NaN to a float -> integer conversion (undefined in C++); it now picks 0 by comparison first, on all sides.

That the check can fail: six mutations of the chain, the sampler and the store, each applied once to a scratch copy, each failing tests of this file and of
tests/test_display_gpu.py; DESIGN.md section 1 lists them with the tests that failed.
"""
import json
import os

import numpy as np
import pytest

from tests import display_kat_io as io, ref

needs_ref = pytest.mark.skipif(not ref.available(), reason="needs /root/reference (or a prebuilt oracle/_ref/libref.so)")


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def tol():
    with open(os.path.join(io.GOLDEN, "display_kat_tol.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def legs(kat):
    """every run and edge run through the oracle and (where it exists) the compiled reference, once"""
    out = {}
    for run in io.runs(kat) + io.edges(kat):
        f, c = io.orc_tonemap(run)
        out[run.key] = {"run": run, "orc": f, "orc8": c, "ref": io.ref_tonemap(run) if ref.available() else None}
    return out


def sides(entry):
    return [(s, entry[s]) for s in ("orc", "ref") if entry[s] is not None]


def test_fixture_is_what_the_issue_asks_for(kat):
    from tests.test_oracle_vs_ref import TM_CASES, tonemapper
    assert float(kat["SPREAD"]) == 1e-5
    for k, case in enumerate(TM_CASES):  # the first seven cases are TM_CASES, field by field
        want, (got, _) = tonemapper(**case), io.tonemapper(kat, f"tm{k}")
        assert bytes(want) == bytes(got), f"tm{k}"
    sizes = {(im.W, im.H) for im in io.images(kat) if (im.num, im.den) == (1, 1)}
    assert sizes >= {(1, 1), (1, 5), (5, 1), (2, 2), (3, 2), (5, 3), (33, 17), (67, 33), (75, 41), (64, 64), (130, 66)}
    assert {(im.w, im.h, im.W, im.H, im.den) for im in io.images(kat) if im.num < im.den} == {(37, 26, 75, 53, 2), (25, 17, 75, 53, 3)}
    assert {(im.num, im.den) for im in io.images(kat) if im.num > im.den} == {(5, 4), (2, 1)}  # zoom > 1: REPEAT addressing, and a positive lambda_base
    assert io.Image(kat, "130x66").levels == 8
    m = kat["master"]
    assert m[..., :3].min() < 2e-3 and m[..., :3].max() > 50 and m[..., 3].std() > 0.1 and np.isfinite(m).all()
    for total, dropped in kat["case_counts"]:
        assert dropped <= 0.05 * total
    per_case = {}
    for run in io.runs(kat):
        n = per_case.setdefault(run.case, [0, 0])
        n[0] += run.kept.size
        n[1] += int((~run.kept).sum())
        assert not (run.kept & run.round_only).any()
    assert [per_case[str(c)] for c in kat["case_names"]] == kat["case_counts"].tolist()
    exits = np.zeros(8, np.int64)
    for run in io.runs(kat):
        if run.local:
            exits += np.bincount(run.exit[run.kept].astype(np.int64), minlength=8)
    assert (exits >= 50).all() and exits.tolist() == kat["exit_kept"].tolist(), exits
    names = [str(n) for n in kat["edge_names"]]
    for want in ("a black pixel", "an all-black image", "a NaN pixel", "a +Inf pixel", "a -Inf pixel", "a pixel at 3e38"):
        assert any(n.startswith(want) for n in names), want


def test_autoexposure_2_alone_behaves_as_0(kat, legs):
    by = {(e["run"].image.name, e["run"].case): e for e in legs.values() if e["run"].key.startswith("run")}
    n = 0
    for (im, case), e in by.items():
        if case == "ae2":
            for s, f in sides(e):
                io.same_bits(f, by[(im, "plain")][s], f"{s}, {im}: autoExposure = 2 against 0")
            n += 1
    assert n >= 7


@pytest.mark.parametrize("side", ["orc", pytest.param("ref", marks=needs_ref)])
def test_every_mip_level_is_within_the_derived_bound(kat, side):
    for im in io.images(kat):
        got = io.chain_of(side, im.padded())
        assert len(got) == int(np.floor(np.log2(max(im.W, im.H)))) + 1
        io.check_chain(got, im.model_chain(kat), f"{side}, {im.name}")


@pytest.mark.parametrize("side", ["orc", pytest.param("ref", marks=needs_ref)])
def test_power_of_two_chain_is_the_box_average(kat, side):
    im = io.Image(kat, "64x64")
    box = [im.render.astype(np.float64)]
    while box[-1].shape[0] > 1:
        b = box[-1]
        box.append((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2]) / 4.0)
    io.check_chain(io.chain_of(side, im.render), [b.astype(np.float32) for b in box], f"{side}, 2 x 2 box averages")
    io.check_chain([b.astype(np.float32) for b in box], im.model_chain(kat), "the model's chain against the box averages")


@needs_ref
def test_chains_of_oracle_and_reference_are_bit_identical(kat):
    for im in io.images(kat):
        for lod, (a, b) in enumerate(zip(io.chain_of("orc", im.padded()), io.chain_of("ref", im.padded()))):
            io.same_bits(a, b, f"{im.name} level {lod}")


@pytest.mark.parametrize("side", ["orc", pytest.param("ref", marks=needs_ref)])
def test_fragcolor_is_within_four_times_the_references_error(kat, tol, legs, side):
    assert tol["SPREAD"] == float(kat["SPREAD"])
    worst = {}
    for e in legs.values():
        run = e["run"]
        if not run.key.startswith("run"):
            continue
        err = gen_measure(e[side], run.frag)
        assert np.isfinite(err[run.kept]).all(), f"{side}, {run.label}: a kept pixel is NaN or infinite on one side only"
        worst[run.case] = max(worst.get(run.case, 0.0), float(err[run.kept].max()))
    for case, w in worst.items():
        rec = tol["cases"][case]["max_error"]
        assert rec <= 1e-3
        print(f"{side} {case:12s} worst {w:.3e}, recorded {rec:.3e}")
        assert w <= 4 * rec, f"{side}, case {case}: {w:.3g} against the model, the reference's own error is {rec:.3g}"


def gen_measure(got, want):
    return io.gen.measure(got, want)


@pytest.mark.parametrize("side", ["orc", pytest.param("ref", marks=needs_ref)])
def test_local_exposure_exit_matches_the_model(kat, tol, legs, side):
    observed = np.zeros(8, np.int64)
    for e in legs.values():
        run = e["run"]
        if not (run.key.startswith("run") and run.local):
            continue
        bound = 4 * tol["cases"][run.case]["max_error"]
        err = io.recovered_exit_errors(e[side], run, run.image.model_chain(kat))  # (8, H, W)
        mine = np.take_along_axis(err, run.exit.astype(np.int64)[None], 0)[0]
        k = run.kept
        assert (mine[k] <= bound).all() and (mine[k] <= err.min(0)[k]).all(), f"{side}, {run.label}: a kept pixel is explained better by another exit than the model's"
        others = np.where(np.arange(8)[:, None, None] == run.exit[None], np.inf, err).min(0)
        observed += np.bincount(run.exit[k & (others > 2 * bound)].astype(np.int64), minlength=8)
    print(f"{side}: kept pixels whose exit is observable, per exit {observed.tolist()}")
    assert (observed >= 50).all(), observed


@pytest.mark.parametrize("side", ["orc", pytest.param("ref", marks=needs_ref)])
def test_codes_equal_the_models(kat, legs, side):
    for e in legs.values():
        run = e["run"]
        io.check_codes(io.quantise(e[side]), run, side)
        if side == "orc":
            io.same_bits(io.quantise(e[side]), e["orc8"], f"{run.label}: the oracle's own RGBA8 against its floats through the store")


def test_store_is_defined_for_every_float():
    """the project's store and the model's: 0.0 and 1.0 exact, every k / 255 stores k, nearest integer, clamped, infinities clamp, NaN (either sign, any payload) -> 0"""
    x = np.array([0.0, -0.0, 1.0, 0.51 / 255, 0.49 / 255, 254.49 / 255, 2.0, -1.0, np.inf, -np.inf, np.nan, -np.nan, 3e38, 1e-45], np.float32)
    x = np.concatenate([x, np.array([0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32).view(np.float32), (np.arange(256, dtype=np.float32) / np.float32(255.0))])
    want = [0, 0, 255, 1, 0, 254, 255, 0, 255, 0, 0, 0, 255, 0, 0, 0, 0] + list(range(256))
    got = io.quantise(x)
    assert got.tolist() == want and io.gen.unorm8(x).tolist() == want


@needs_ref
def test_oracle_and_reference_are_bit_identical_on_every_stored_pixel(legs):
    for e in legs.values():
        io.same_bits(e["orc"], e["ref"], e["run"].label)


def test_edge_runs_store_zero_where_the_image_goes_nan(kat, legs):
    n = 0
    for e in legs.values():
        run = e["run"]
        if run.key.startswith("edge") and "no exposure" not in run.label and any(t in run.label for t in ("NaN", "Inf", "all-black")):
            for s, f in sides(e):
                assert (io.quantise(f)[..., :3] == 0).all(), f"{s}, {run.label}"
            assert (e["orc8"][..., :3] == 0).all() and (run.code[..., :3] == 0).all()
            n += 1
    assert n == 8

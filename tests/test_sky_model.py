"""The procedural sun & sky (csrc/pt_sky.h sun_and_sky, oracle/orc_sky.h, the reference's shaders/sun_and_sky.glsl) held to the INDEPENDENT float64 model of
tests/golden/gen_sky_kat.py, direction by direction: 23 settings rows (the six variants of tests/test_oracle_vs_ref.py and one hand-made row per branch that no
committed sky input reached before) x sphere, horizon-band, sun-fan and at-the-sun directions, 48691 rows.

Legs: the oracle through orc_sun_and_sky and through orc_shading_probe case SUN_AND_SKY, the compiled reference (ref_sun_and_sky), the product's host build
of pt_sky.h through th_shading_probe.  Each is within 4 x the error the compiled reference shows against the model ON ITS CLASS of rows
(tests/golden/sky_kat_tol.json, written by measure_sky_kat.py, never taken from the product) on the kept rows, and all are bit-identical to each other on
EVERY row.  tests/test_sky_gpu.py holds the device to the same fixture.  The error measure is the fixture's: max over the channels of |got - want| over max
over the channels of |want|.

WHAT IT FOUND.  No leg is outside its bound and no two legs differ.  Reported, not changed (GLSL leaves acos undefined there and all legs agree): on 71 of
the 403 rows that look at the sun from within 1e-3 rad, the float32 dot(real_dir, real_sun) of sun_and_sky.glsl:523 exceeds 1, acos answers NaN,
`sun_angle < sun_radius` fails and the disc vanishes on exactly that ray (the sky alone is returned: 1.6 where the model says 4681).  numpy's float32 dot
rounds some of these rows to exactly 1 where the legs' exceeds it, so the fixture's rule is about every evaluation order: a row whose float64 cosine is
above 1 - 2^-21 is never kept (gen_sky_kat.DOT_MARGIN).  The reference also showed that numpy's float32 agreeing with float64 is luck in the smoothstep's
rise (its own acos and dot put it at 4e-3 there): a row is kept only when moving the cosine by 2^-23 in the float64 model stays within the spread
(gen_sky_kat.DOT_NUDGE).

PROOF THAT THE CHECK CAN FAIL.  The model was broken one rule at a time (gen_sky_kat.BREAK), re-minted in a scratch copy, and the unchanged oracle run
against it; the bounds are 4 x the recorded maxima, 7.4e-6 (outside) .. 5.0e-4 (core of a physically scaled sun).  Largest error of the oracle against the
broken model, the class that shows it, and the classes out of their bound:
    one digit of a Perez coefficient (y, E: 0.053919)   1.89e-03 sphere    all nine
    zenith x and y swapped                               3.38e-01 sphere    all nine
    one entry of the XYZ -> RGB matrix (0.042 -> 0.142)  1.47e-01 sphere    all nine
    tan(chi) replaced by chi                             1.98e-01 sphere    all nine
    irradiance mean over 16 instead of 25                3.61e-01 rise      all nine (every class has rows below the horizon)
    y_is_up swizzle dropped                              1.33e+01 outside   all nine
    night factor squared once                            7.35e-01 rim       all nine
    glow exponent 2                                      3.82e-01 sphere    all but outside
    smoothstep edges 8.5 and 9.5 without haze / 50       2.14e-01 core, physically scaled; sphere, core, rise, sun
    disc radius without the factor 10                    1.67e+03 glow      all but core and rise (no row of theirs is inside the small radius)
    `target -= max_glow` dropped                         4.74e-01 rise      sphere, core physically scaled, rise, sun
    the ground blend's dn unclamped                      1.26e+01 sphere    all but core
    redblueshift sign                                    6.64e-01 core, physically scaled; all nine
    the cos_gamma > 1 fold dropped                       0        none: acos of :523 is undefined on every row that reaches the fold, so none is kept; the
                                                                  fold is held by bit-identity with the reference alone
The same kind of break planted in the product's csrc/pt_sky.h (host build only, scratch copy) against the committed fixture:
    Perez y, E: 0.052919 -> 0.053919                     1.89e-03 sphere    all nine
    night factor squared once                            2.78e+00 sphere    all nine
    smoothstep edges 8.5, 9.5 without haze / 50          5.25e-02 rise      sphere, rise, sun
    irradiance mean over 16                              5.65e-01 rise      all nine
"""
import os
import re

import numpy as np
import pytest

from tests import orc, ref, sky_kat_io as io


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def gen():
    return io.generator()


@pytest.fixture(scope="module")
def tol():
    return io.tolerances()


@pytest.fixture(scope="module")
def oracle_out(kat):
    out = io.through_probe(orc.lib().orc_shading_probe)(kat["rows"])
    out.setflags(write=False)
    return out


LARGEST_FIXTURE_BEFORE = 974864   # bytes of display_kat.npz, the largest file of tests/golden/ before this fixture was added: no new file may pass it


def host_probe():
    from tests import host_harness
    return host_harness.lib().th_shading_probe


# ---- the fixture itself ----------------------------------------------------------------------------------------------------------------------------------------
def test_generator_is_independent_and_deterministic(tmp_path, gen):
    src = open(os.path.join(io.GOLDEN, "gen_sky_kat.py")).read()
    imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, re.M)
    assert set(imports) <= {"os", "sys", "numpy", "gen_float_kat", "gen_surface_kat"}, imports   # nothing of oracle/, tests/, vk_raytrace_amd/
    assert len(re.findall(r"#.*?:\d+(-\d+)?", src)) >= 30   # shader lines cited per rule
    out = str(tmp_path / "again.npz")
    gen.main(out, caps=False)
    assert open(out, "rb").read() == open(os.path.join(io.GOLDEN, "sky_kat.npz"), "rb").read()
    assert os.path.getsize(out) <= LARGEST_FIXTURE_BEFORE


def test_settings_rows_are_the_variants_and_the_named_branches(kat, gen):
    from tests.test_oracle_vs_ref import sunsky_variants
    from tests.test_float_kat import sky_rows
    for k, ss in enumerate(sunsky_variants()):
        assert bytes(ss) == kat["settings"][k].tobytes(), f"settings row {k} is not sunsky_variants()[{k}]"
    fk = io.float_kat_io.load()
    assert np.array_equal(kat["sphere"], fk["sky_dirs"])
    # the six variants x 1508 directions of tests/test_float_kat.py are rows of this fixture, word for word
    mine = kat["rows"][(kat["row_setting"] < 6) & (kat["row_class"] == gen.C_SPHERE)]
    assert np.array_equal(mine.view(np.uint32), sky_rows(fk).view(np.uint32))
    words = kat["settings"]
    yup, phys = words.view(np.int32)[:, gen.W_YUP], words.view(np.int32)[:, gen.W_PHYS]
    assert set(yup) == {0, 1} and set(phys) == {0, 1} and (words[:, gen.W_HH] != 0).sum() >= 2
    pair = words[6].copy()   # physically_scaled_sun 0 and 1 with otherwise equal settings
    pair.view(np.int32)[gen.W_PHYS] = 1
    assert np.array_equal(pair, words[0])
    unit = np.linalg.norm(words[:, gen.W_SUN:gen.W_SUN + 3].astype(np.float64), axis=1)
    assert (np.abs(unit - 1) < 1e-6).any() and (np.abs(unit - 1) > 1e-3).any()   # a unit sun_direction, and the default, which is none


def test_fixture_meets_the_caps(kat, gen, tol):
    """sphere, horizon, glow, rim, outside at most 2 % dropped; core >= 50 kept under physically_scaled_sun == 0; the physically scaled core >= 50; rise >= 30;
    every branch of BRANCHES >= 50 kept rows; the tolerance file was measured on this fixture and passes the guard rail"""
    per_class, per_branch = gen.check_caps(kept_view(kat))
    assert list(kat["branch_names"]) == list(gen.BRANCHES) and list(kat["class_names"]) == list(gen.CLASSES) and str(kat["measure"]) == gen.MEASURE
    for c in gen.DROP_CAPPED:
        rows, kept = per_class[c]
        assert rows >= 400 and rows - kept <= 0.02 * rows
    assert min(per_branch.values()) >= 50
    assert per_class["rise"][1] >= 30 and per_class["core"][1] >= 50 and per_class["core, physically scaled"][1] >= 50
    fan = np.isin(kat["row_class"], [gen.C_CORE, gen.C_CORE_PHYS, gen.C_RISE, gen.C_GLOW, gen.C_RIM, gen.C_OUTSIDE])
    assert (np.bincount(kat["row_setting"][fan]) >= 400).all()   # at least 400 fan directions per settings row
    assert np.isfinite(kat["want"][kat["kept"]]).all() and not (kat["kept"] & kat["at_sun"]).any()
    assert np.array_equal(kat["class_spread"], [gen.SPREADS[c] for c in gen.CLASSES]) and float(kat["SPREAD"]) == gen.fk.SPREAD
    assert tol["rows"] == len(kat["rows"]) and tol["measure"] == gen.MEASURE
    for k, name in enumerate(gen.CLASSES):
        t = tol["classes"][name]
        m = kat["row_class"] == k
        assert (t["kept"], t["dropped"], t["spread"]) == (int((m & kat["kept"]).sum()), int((m & ~kat["kept"]).sum()), gen.SPREADS[name]), "sky_kat_tol.json was measured on another fixture"
        assert t["max_error"] <= 1e-3   # the project's parity bar: a larger recorded maximum rejects the fixture


def kept_view(kat):
    return {k: kat[k] for k in ("row_class", "kept", "branches", "class_names", "branch_names", "settings", "row_setting")}


# ---- the CPU legs ----------------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_within_the_bounds_through_both_entries(kat, tol, oracle_out):
    io.check(kat, tol, oracle_out, "oracle")
    direct = io.through_call(orc.lib().orc_sun_and_sky)(kat["rows"])
    assert io.same_bits(direct, oracle_out) == 0, "orc_sun_and_sky and orc_shading_probe case SUN_AND_SKY differ"
    assert not np.isnan(oracle_out[~kat["at_sun"]]).any() and oracle_out.max() > 100   # the disc is there


@pytest.mark.skipif(not ref.available(), reason="needs the reference tree (or a prebuilt oracle/_ref/libref.so)")
def test_reference_within_the_bounds_and_equal_to_the_oracle(kat, tol, oracle_out):
    got = io.through_call(ref.lib().ref_sun_and_sky)(kat["rows"])
    io.check(kat, tol, got, "reference")
    bad = io.same_bits(got, oracle_out)
    assert bad == 0, f"compiled reference and oracle differ in {bad} values"


def test_host_build_within_the_bounds_and_equal_to_the_oracle(kat, tol, oracle_out):
    got = io.through_probe(host_probe())(kat["rows"])
    io.check(kat, tol, got, "host")
    bad = io.same_bits(got, oracle_out)
    assert bad == 0, f"host build of pt_sky.h and oracle differ in {bad} values"   # every row: ill-conditioned ones and the rays at the sun included


def test_the_ray_at_the_sun_loses_the_disc_on_every_leg_alike(kat, gen, oracle_out):
    """the reported quirk (docstring): where the float32 dot exceeds 1 the legs return the sky without the disc.  Not an expectation of the model -- those rows
    are never kept -- but pinned here so that a change of it is seen: at least one row of every settings row with a disc is inside 1e-3 rad of the sun, and on
    some of them the oracle is far below the model's disc"""
    at_sun = kat["at_sun"]
    words = kat["settings"][kat["row_setting"]]
    disc = (words[:, gen.W_DISK_I] > 0) & (words[:, gen.W_DISK_S] > 0) & (words[:, gen.W_MULT] > 0)
    assert set(kat["row_setting"][at_sun & disc]) == set(kat["row_setting"][disc])
    e = io.errors(kat, oracle_out)
    lost = at_sun & disc & (e > 0.5)
    print(f"{int(lost.sum())} of {int(at_sun.sum())} rows at the sun lose the disc")
    assert lost.any() and not (lost & kat["kept"]).any()

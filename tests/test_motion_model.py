"""Motion of moving instances: the host build of vk_raytrace_amd/csrc/pt_motion.h (tests/motion_host.py) against the float64
model of the definition (tests/golden/gen_motion_kat.py), its exact properties, and a check of the table's direction that shares nothing with the
model's reading of it.  No GPU: tests/test_motion_gpu.py holds the device to this host build bit for bit.

The bound is section 5.3's, derived and not measured: the model's float64 run carries the running first-order error bound of gen_temporal_kat.V, and
the two affine products (toPrev on the point, normalToPrev on the normal) and the unit of the insertion are made of V's operations, so they extend
it by their own rules -- three products and three sums per row with u |result| each, the unit's quotient and square root -- with nothing added by
hand.  The table's words are inputs both runs share (each the float64 product rounded once); the host's table has to equal the model's on every bit.
Applied as it stands, with the 2^-20 slack of tests/test_temporal_model.py.  measure_motion_kat.py records the host build's worst ratio in
motion_kat_tol.json: reported, not used.  A case may drop at most 5 % of its pixels (section 5.3's cap; the moves were chosen under it).

Planted breaks (test_a_planted_break_fails_its_test applies each to scratch copies of the headers, never to the tree, and runs the named check):
    toPrev inverted                       history_taps_hit_the_same_object_point (slide)
    normal matrix not transposed          host_meets_model (yaw)
    bound test after the table read       hostile_planes_sanitized (the stand-alone program under -fsanitize=address,undefined)
    `moved` ignored                       moved_is_a_matter_of_objectToWorld_alone
    Hg' storing g'                        host_meets_model (yaw): the stored guide is the current frame's
    t_exp taken from P                    host_meets_model (reveal)
"""
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import motion_host as mh, svgf_host as sh, temporal_host as th
from tests import test_temporal_model as tmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_motion_kat", os.path.join(ROOT, "tests", "golden", "gen_motion_kat.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
gen, bits, SLACK = mk.gen, tmodel.bits, tmodel.SLACK
CASES = [(size, move) for size in mk.SIZES for move in mk.MOVES]
ASAN_MAIN = os.path.join(ROOT, "tests", "cpp", "motion_asan_main.cpp")

_judged = {}


def judged(size, move):
    """the model's inputs and verdict of a case, computed once and shared"""
    if (size, move) not in _judged:
        inp = mk.case_inputs(size, move)
        _judged[size, move] = (inp, mk.judge(inp))
    return _judged[size, move]


def host_table(inp, L=None):
    return mh.table(inp["hist_words"], inp["cur_words"], L)


def run_host(inp, L=None, ids=None, tab=None, moments=False, hist="own"):
    hist = tmodel.history_of(inp) if isinstance(hist, str) else hist
    rc, new, pr = mh.temporal_moving(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], tmodel.params_of(inp), inp["ids"] if ids is None else ids,
                                     host_table(inp, L) if tab is None else tab, hist, moments=moments, want_probe=True, L=L)
    assert rc == 0
    return new, pr


def run_static(inp):
    rc, new = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], tmodel.params_of(inp), tmodel.history_of(inp))
    assert rc == 0
    return new


def same_pixels(a, b):
    """(H, W) mask: colour, guide and length equal on every bit"""
    return (bits(a.colour) == bits(b.colour)).all(-1) & (bits(a.guide) == bits(b.guide)).all(-1) & (bits(a.length) == bits(b.length))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_meets_its_caps():
    """every case drops at most 5 % of its pixels in the model's own two runs; the history is the temporal fixture's; every move but `none` applies the
    table to the box's pixels and to nothing else; `reveal` bares its old place"""
    for size, move in CASES:
        inp, r = judged(size, move)
        w, h = size
        mk.drop_report({f"{size} {move}": r})
        g1, g2 = gen.guides(gen.moved("none", w / h), w, h)
        assert np.array_equal(bits(inp["hist"]["guide"][..., :3]), bits(g1[..., :3])) and np.array_equal(bits(inp["hist"]["guide"][..., 3]), bits(g2[..., 0]))
        on_box = inp["ids"].reshape(-1) == mk.BOX_ID
        assert on_box.sum() > 0.05 * w * h
        assert np.array_equal(r["applied"], on_box if move != "none" else np.zeros(w * h, bool))
        if move == "reveal":
            bared = (inp["hist"]["ids"].reshape(-1) == mk.BOX_ID) & ~on_box
            assert bared.sum() > 0.05 * w * h and (r["outcome"][bared & r["kept"]] >= gen.CURRENT).mean() > 0.9
        if move in ("slide", "yaw", "mirror"):
            assert (r["outcome"][on_box & r["kept"]] <= gen.HISTORY_ONLY).mean() > 0.9     # the moved box keeps its history


@pytest.mark.parametrize("move", mk.MOVES)
def test_the_host_table_is_the_models(move):
    inp, _ = judged((45, 37), move)
    tab = host_table(inp)
    assert np.array_equal(bits(tab[:, :12].reshape(-1, 3, 4)), bits(inp["toPrev"]))
    assert np.array_equal(bits(tab[:, 12:24].reshape(-1, 3, 4)[:, :, :3]), bits(inp["normalToPrev"])) and not bits(tab[:, 12:24].reshape(-1, 3, 4)[:, :, 3]).any()
    assert np.array_equal(mh.moved_bits(tab), inp["moved"].astype(np.uint32)) and not bits(tab[:, 25:]).any()


# ---- host build against model ----------------------------------------------------------------------------------------------------------------------------------
def check_host_meets_model(size, move, L=None):
    inp, r = judged(size, move)
    new, pr = run_host(inp, L)
    worst, classes, exact = tmodel.ratios(inp, r, new, pr)
    assert classes, f"{size} {move}: outcome classes differ on kept pixels"
    assert exact, f"{size} {move}: a pixel without history is not the current pixel bit for bit"
    assert all(v <= 1.0 for v in worst.values()), f"{size} {move}: error / bound {worst}"
    # step 4 and the stored guide are the current frame's
    assert np.array_equal(bits(new.colour[..., 3]), bits(inp["colour"][..., 3]))
    assert np.array_equal(bits(new.guide[..., :3]), bits(inp["g1"][..., :3])) and np.array_equal(bits(new.guide[..., 3]), bits(inp["g2"][..., 0]))
    # the depth the taps are tested against is P''s: within 1e-5 of the model's, the margin every decision on it has (fp32 rounds the few dozen operations up
    # to it an order of magnitude below that; a depth taken from the unmoved P is off by the move)
    n = inp["w"] * inp["h"]
    at = r["kept"] & r["reached"]
    t_exp = pr["point"].reshape(n, 4)[:, 3].astype(np.float64)
    assert (np.abs(t_exp[at] - r["t_exp"][at]) <= 1e-5 * r["t_exp"][at]).all(), f"{size} {move}: t_exp"
    return worst


@pytest.mark.parametrize("size,move", CASES, ids=[f"{s[0]}x{s[1]}-{m}" for s, m in CASES])
def test_host_meets_model(size, move):
    check_host_meets_model(size, move)


# ---- from outside the model --------------------------------------------------------------------------------------------------------------------------------------
def check_history_taps_hit_the_same_object_point(move, L=None):
    """For the pixels of the moved box whose history was found: the point of the OBJECT that each counted history tap shows -- the history camera's hit point
    at the tap, the box being at its history pose -- is the point of the object the current pixel shows -- its hit point taken back through the box's current
    pose -- within the tap's footprint (the largest distance to the hit points of its eight neighbours on the box).  Both from the fixture's analytic hit
    points, in float64: the table is not consulted.  A toPrev applied in the wrong direction is off by twice the move."""
    size = (96, 64)
    w, h = size
    inp, r = judged(size, move)
    _, pr = run_host(inp, L)
    n = w * h
    cur_obj = (np.linalg.inv(inp["box"]) @ np.concatenate([inp["points"], np.ones((n, 1))], 1).T).T[:, :3]
    hist_obj, hist_ids = inp["hist"]["points"], inp["hist"]["ids"].reshape(-1)
    foot = np.zeros(n)
    ys, xs = np.divmod(np.arange(n), w)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qx, qy = np.clip(xs + dx, 0, w - 1), np.clip(ys + dy, 0, h - 1)
            q = qy * w + qx
            foot = np.maximum(foot, np.where(hist_ids[q] == mk.BOX_ID, np.linalg.norm(hist_obj[q] - hist_obj, axis=1), 0.0))
    on_box = (inp["ids"].reshape(-1) == mk.BOX_ID) & r["kept"]
    counted = pr["verdicts"].reshape(n, 4) == th.COUNTED
    taps = pr["taps"].reshape(n, 4, 2)
    checked = 0
    for i in range(4):
        sel = on_box & counted[:, i]
        q = taps[sel, i, 1] * w + taps[sel, i, 0]
        assert (hist_ids[q] == mk.BOX_ID).all(), f"{move}: a counted tap of a box pixel is not on the box"
        dist = np.linalg.norm(hist_obj[q] - cur_obj[sel], axis=1)
        assert (dist <= 1.05 * foot[q] + 1e-6).all(), f"{move}: tap {i} shows another point of the box: worst {np.max(dist / (foot[q] + 1e-6)):.2f} footprints"
        checked += int(sel.sum())
    assert checked > 0.8 * on_box.sum(), (checked, int(on_box.sum()))


@pytest.mark.parametrize("move", ["slide", "yaw", "scale", "mirror", "slide_camera"])
def test_history_taps_hit_the_same_object_point(move):
    check_history_taps_hit_the_same_object_point(move)


# ---- exact properties ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", mk.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_without_a_move_the_moving_form_is_the_static_one_bit_for_bit(size):
    """colour, guide, length and, with tracking on, the moments"""
    inp, _ = judged(size, "none")
    new, _ = run_host(inp)
    assert same_pixels(new, run_static(inp)).all()
    H = inp["hist"]
    rng = np.random.default_rng(11)
    hm = np.exp(rng.uniform(-3, 3, (size[1], size[0], 2))).astype(np.float32)
    hist = sh.History(H["colour"], H["guide"], H["length"], hm, H["worldToClip"], H["eye"])
    rc, want = sh.temporal_m(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], tmodel.params_of(inp), hist)
    assert rc == 0
    got, _ = run_host(inp, moments=True, hist=mh.History(H["colour"], H["guide"], H["length"], H["worldToClip"], H["eye"], hm))
    assert same_pixels(got, want).all() and np.array_equal(bits(got.moments), bits(want.moments))


def test_a_first_call_is_the_static_first_call():
    inp, _ = judged((45, 37), "slide")
    rc, new = mh.temporal_moving(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], tmodel.params_of(inp), inp["ids"], host_table(inp), None)
    rc2, want = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], tmodel.params_of(inp), None)
    assert rc == 0 == rc2 and same_pixels(new, want).all() and np.array_equal(bits(new.colour), bits(inp["colour"]))


def check_moved_is_a_matter_of_objectToWorld_alone(L=None):
    """moved is 1 exactly when a bit of objectToWorld differs: a sign of zero counts, worldToObject does not -- and a record whose moved is 0 is not applied,
    whatever its matrices hold"""
    inp, _ = judged((45, 37), "slide")
    cur = inp["hist_words"].copy()
    cur[mk.BOX_ID, 12:] = np.array([7.0, -3.0, 1e6, 4.0, 0.0, 0.0, 0.0, 1e9, np.nan, 2.0, 2.0, -5.0], np.float32)     # worldToObject only
    tab = mh.table(inp["hist_words"], cur, L)
    assert not mh.moved_bits(tab).any()
    new, _ = run_host(inp, L, tab=tab)
    assert same_pixels(new, run_static(inp)).all()
    cur = inp["hist_words"].copy()
    cur[mk.FLOOR, 3] = np.float32(-0.0)          # objectToWorld: +0 -> -0
    assert mh.moved_bits(mh.table(inp["hist_words"], cur, L)).tolist() == [1, 0, 0]


def test_moved_is_a_matter_of_objectToWorld_alone():
    check_moved_is_a_matter_of_objectToWorld_alone()


def hostile_ids(inp, rng):
    """the case's plane with a third of its words replaced: numInstances, 0x7fffffff, NONE and random words that name no instance"""
    ids = inp["ids"].copy().reshape(-1)
    n = ids.size
    pick = rng.uniform(size=n) < 0.33
    words = rng.integers(mk.NUM_INSTANCES, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    kind = rng.integers(0, 4, n)
    hostile = np.where(kind == 0, np.uint32(mk.NUM_INSTANCES), np.where(kind == 1, np.uint32(0x7FFFFFFF), np.where(kind == 2, np.uint32(mk.NONE), words))).astype(np.uint32)
    return np.where(pick, hostile, ids).astype(np.uint32).reshape(inp["ids"].shape), pick.reshape(inp["ids"].shape)


@pytest.mark.parametrize("move", ["slide", "mirror"])
def test_hostile_planes_give_the_static_form(move):
    inp, _ = judged((45, 37), move)
    ids, pick = hostile_ids(inp, np.random.default_rng(3))
    new, _ = run_host(inp, ids=ids)
    honest, _ = run_host(inp)
    static = run_static(inp)
    assert pick.sum() > 300 and same_pixels(new, static)[pick].all() and same_pixels(new, honest)[~pick].all()
    assert not same_pixels(honest, static)[inp["ids"] == mk.BOX_ID].all()       # (the table does change the box's pixels)


def check_hostile_planes_sanitized(header_dir=None):
    """tests/cpp/motion_asan_main.cpp: temporal_pixel_moving over hostile planes and tables in a stand-alone program built with
    -fsanitize=address,undefined, the table in a heap block of exactly numInstances records"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "motion_asan")
        subprocess.check_call(["g++"] + ([] if header_dir is None else ["-I" + header_dir]) + [c for c in mh.COMPILE if c not in ("-fopenmp", "-fPIC")]
                              + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, ASAN_MAIN])
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 0 and "pixels" in p.stdout, (p.stdout + p.stderr)[-600:]


def test_hostile_planes_sanitized():
    check_hostile_planes_sanitized()


# ---- planted breaks ----------------------------------------------------------------------------------------------------------------------------------------------
MOTION, TEMPORAL = "pt_motion.h", "pt_temporal.h"
BREAKS = {
    "to_prev_inverted": ([(MOTION, "motion_compose(hist, cur + 12, r, c)", "motion_compose(cur, hist + 12, r, c)")],
                         lambda L, d: check_history_taps_hit_the_same_object_point("slide", L)),
    "normal_not_transposed": ([(MOTION, "motion_compose(cur, hist + 12, c, r)", "motion_compose(cur, hist + 12, r, c)")], lambda L, d: check_host_meets_model((96, 64), "yaw", L)),
    "bound_after_read": ([(MOTION, "if(i < numInstances && table[i].moved)", "if(table[i].moved && i < numInstances)")], lambda L, d: check_hostile_planes_sanitized(d)),
    "moved_ignored": ([(MOTION, "if(i < numInstances && table[i].moved)", "if(i < numInstances)")], lambda L, d: check_moved_is_a_matter_of_objectToWorld_alone(L)),
    "stored_guide_is_moved": ([(TEMPORAL, "o.guide  = DnPx{g1.x, g1.y, g1.z, t};", "o.guide  = DnPx{gn.x, gn.y, gn.z, t};")], lambda L, d: check_host_meets_model((96, 64), "yaw", L)),
    "t_exp_from_unmoved_point": ([(MOTION, "temporal_resolve(src, k, c, g1, t, ox, oy, oz, q, gn,", "temporal_resolve(src, k, c, g1, t, Px, Py, Pz, q, gn,"),
                                  (TEMPORAL, "Px - k.eyeH[0], ey = Py - k.eyeH[1], ez = Pz - k.eyeH[2]", "ox - k.eyeH[0], ey = oy - k.eyeH[1], ez = oz - k.eyeH[2]")],
                                 lambda L, d: check_host_meets_model((96, 64), "reveal", L)),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_a_planted_break_fails_its_test(name):
    edits, check = BREAKS[name]
    with tempfile.TemporaryDirectory() as tmp:
        for header in (MOTION, TEMPORAL, "pt_svgf.h"):      # (pt_svgf.h: so that its include of pt_temporal.h finds the copy)
            text = open(os.path.join(mh.CSRC, header)).read()
            for _, old, new in [e for e in edits if e[0] == header]:
                assert text.count(old) == 1, (name, old)
                text = text.replace(old, new)
            open(os.path.join(tmp, header), "w").write(text)
        L = None if name == "bound_after_read" else mh.bind(mh.compile_to(os.path.join(tmp, "libbroken.so"), header_dir=tmp))
        with pytest.raises((AssertionError, subprocess.CalledProcessError)):
            check(L, tmp)

"""The candidate walk (trace contract T3 - T6) and stochastic alpha on the CPU, held to the independent model of tests/golden/gen_walk_kat.py: a
brute force over every world triangle in float64, written from the shader text, with a kept mask the model decides alone (tests/walk_kat_io.py holds the rules).

Legs, on one scene built from the fixture's arrays:
  the oracle                 orc.trace_closest (closest hit and the seed afterwards), again with use_any_hit(0); and the frame the device test renders
  the query host build       pt_query.h's query_ray (tests/cpp/query_host.cpp): CLOSEST, OCCLUDED in both variants, CANDIDATES with 16 results per ray against the
                             model's key list before alpha -- flat and two-level structure, merge_singles on and off
  TracedScene.settle         exact = 0 (the lock-step two-pass of pt_settle.h), 1 (the exact key-ordered loop: a leg here, not the definition) and 2 (the trace
                             machine), closest and bounded shadow, both structures; once more on compact nodes
  any-hit off                the host harness has no switch for pt_use_any_hit(0): the query host build runs on a copy of the scene with alphaMode 0 on every
                             material, which sets TRI_OPAQUE on every instance as the switch does
The fixture's zero-draw rays (a draw of exactly 0.0 on a zero-opacity candidate or on the certain hit's own draw) send every two-pass leg through its exact
fallback: settle_draws / consume_rejected_draws return false on them by construction.

tools/walk_mutations.py breaks the product ten ways in a scratch copy; each must fail a test of this file.  The generator's BREAK list holds the model-side
counterparts, and test_a_broken_model_disagrees_with_the_fixture checks that the comparison can fail from that side too."""
import os

import numpy as np
import pytest

from tests import walk_kat_io as io
from tests.host_harness import NONE, TracedScene
from tests.test_query_host import CANDIDATES, CLOSEST, OCCLUDED, host_query
from vk_raytrace_amd import capi

VARIANTS = (capi.PT_VARIANT_RAYQUERY, capi.PT_VARIANT_RTX)


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def gen():
    return io.generator()


def test_fixture_is_what_the_generator_mints(kat, gen, tmp_path):
    """deterministic and byte-identical; under the size limit; the caps hold: at most 10 % of any ray family dropped, 50 kept rays per tag (4 for the exact-row and
    zero-draw tags); the census is the one the generator's docstring records"""
    path = str(tmp_path / "walk_kat.npz")
    gen.main(path)
    committed = os.path.join(io.GOLDEN, "walk_kat.npz")
    assert open(path, "rb").read() == open(committed, "rb").read()
    assert os.path.getsize(committed) < 1 << 20
    drops, counts = gen.check_caps(kat)
    assert max(drops.values()) <= 0.10
    assert len(kat["world_rec"]) <= 300 and 4097 < len(kat["kept"]) < 5000
    for name, c in counts.items():
        assert f"{name} {c}" in gen.__doc__, f"the census in the generator's docstring does not say: {name} {c}"


def test_zero_draw_rays_sit_where_the_device_test_needs_them(kat):
    """one whole wavefront of 64 lanes holds zero-draw rays only, others share a wavefront with ordinary rays, all inside the first 4097"""
    zero = kat["ray_family"] == io.F_ZERO
    assert zero[128:192].all() and np.nonzero(zero)[0].max() < 4097
    shared = [w for w in range(4097 // 64) if 0 < zero[64 * w:64 * w + 64].sum() < 64]
    assert len(shared) >= 8
    assert kat["kept"][zero].all() and kat["kept"][kat["ray_family"] == io.F_EXACT].all()


@pytest.mark.parametrize("brk", io.generator().BREAK)
def test_a_broken_model_disagrees_with_the_fixture(kat, gen, brk):
    """each rule of BREAK, broken in the model, changes an answer on a KEPT ray of the committed fixture"""
    out = gen.mint(brk)
    keys = ("closest_world", "closest_seed", "closest_draws", "shadow_hit", "shadow_seed", "shadow_seed_rtx", "shadow_draws", "opaque_shadow", "key_world")
    differ = {k: int((kat["kept"] & (out[k] != kat[k]).reshape(len(kat["kept"]), -1).any(1)).sum()) for k in keys}
    print(brk, differ)
    assert sum(differ.values()) > 0, brk


def test_scene_holds_the_fixtures_words(kat):
    sc = io.fixture_scene(kat)
    io.check_scene_words(kat, sc)
    tr = TracedScene(sc)
    assert tr.n == len(kat["world_rec"])
    for w in range(0, tr.n, 7):   # the product's world records are T1's bits
        rec, _ = tr.world_tri(w)
        assert np.array_equal(rec.astype(np.float32).view(np.uint32), kat["world_rec"][w].view(np.uint32)), w
    tr.close()


def test_oracle_closest(kat):
    from tests import orc
    o = orc.Oracle()
    o.set_scene(io.fixture_scene(kat))
    t, node, prim, uv, seeds = o.trace_closest(kat["ray_origin"], kat["ray_direction"], kat["ray_seed"])
    node, prim = node.astype(np.int64), prim.astype(np.int64)
    miss = node < 0
    first = np.concatenate([[0], np.cumsum(np.bincount(kat["world_inst"], minlength=len(kat["node_record"])))])
    world = np.where(miss, -1, first[np.maximum(node, 0)] + prim)
    answered = io.check_closest(kat, "oracle", world, np.stack([t, uv[:, 0], uv[:, 1]], 1), seeds,
                                ids=(np.where(miss, np.int64(NONE), node), np.where(miss, -1, prim), np.where(miss, -1, kat["node_record"][np.maximum(node, 0)].astype(np.int64))))
    io.census(kat, answered)
    o.close()
    o = orc.Oracle()
    o.use_any_hit(False)                 # every triangle opaque: the nearest key, the seed untouched
    o.set_scene(io.fixture_scene(kat))
    t, node, prim, uv, seeds = o.trace_closest(kat["ray_origin"], kat["ray_direction"], kat["ray_seed"])
    node, prim = node.astype(np.int64), prim.astype(np.int64)
    io.check_closest(kat, "oracle, any-hit off", np.where(node < 0, -1, first[np.maximum(node, 0)] + prim), np.stack([t, uv[:, 0], uv[:, 1]], 1), seeds, opaque=True)
    o.close()


@pytest.mark.parametrize("merge_singles", [True, False], ids=["merged", "one BLAS per prim-mesh"])
def test_query_host_build(kat, merge_singles):
    sc = io.fixture_scene(kat)
    tr = TracedScene(sc, merge_singles=merge_singles)
    rays = io.rays(kat)
    for two in (0, 1):
        what = f"query host two={two} merge_singles={merge_singles}"
        answered = io.records_closest(kat, what + " CLOSEST", host_query(tr, two, CLOSEST, rays))
        for variant in VARIANTS:
            answered &= io.records_shadow(kat, what + f" OCCLUDED variant {variant}", host_query(tr, two, OCCLUDED, rays, variant=variant), variant)
        answered &= io.records_candidates(kat, what + " CANDIDATES", host_query(tr, two, CANDIDATES, rays, hits_per_ray=io.KEYS))
        io.census(kat, answered)
    tr.close()


@pytest.mark.parametrize("exact", [0, 1, 2], ids=["two-pass", "exact loop", "trace machine"])
def test_settle(kat, exact):
    """closest and bounded shadow, both structures, both variants: hit, t / u / v, the seed afterwards AND the number of draws"""
    tr = TracedScene(io.fixture_scene(kat))
    settle_legs(kat, tr, exact, f"settle exact={exact}")
    tr.close()


def test_settle_on_compact_nodes(kat):
    tr = TracedScene(io.fixture_scene(kat), compact_nodes=True)
    settle_legs(kat, tr, 2, "settle on compact nodes, trace machine")
    settle_legs(kat, tr, 0, "settle on compact nodes, two-pass")
    tr.close()


def settle_legs(kat, tr, exact, what):
    org, dirs, seeds, tmax = kat["ray_origin"], kat["ray_direction"], kat["ray_seed"], kat["ray_tmax"]
    for two in (0, 1):
        w, tuv, sd, dr = tr.settle(0, two, exact, org, dirs, seeds)
        answered = io.check_closest(kat, f"{what} two={two} closest", w, tuv, sd, draws=dr)
        for variant in VARIANTS:
            w, _, sd, dr = tr.settle(1, two, exact, org, dirs, seeds, tmax, variant)
            answered &= io.check_shadow(kat, f"{what} two={two} shadow variant {variant}", w, sd, variant, draws=dr)
        io.census(kat, answered)


def test_any_hit_off(kat):
    """every triangle opaque: the nearest key commits, nothing draws (the query host build on the all-OPAQUE copy of the scene, see the docstring)"""
    tr = TracedScene(io.fixture_scene(kat, opaque=True))
    rays = io.rays(kat)
    for two in (0, 1):
        what = f"any-hit off two={two}"
        io.records_closest(kat, what + " CLOSEST", host_query(tr, two, CLOSEST, rays), opaque=True)
        for variant in VARIANTS:
            io.records_shadow(kat, what + " OCCLUDED", host_query(tr, two, OCCLUDED, rays, variant=variant), variant, opaque=True)
        io.records_candidates(kat, what + " CANDIDATES", host_query(tr, two, CANDIDATES, rays, hits_per_ray=io.KEYS))
    tr.close()


def test_the_frame_whose_first_traversal_draw_is_zero(kat):
    """the frames case of tests/test_walk_gpu.py, on the oracle: behind a screen-filling BLEND card of factor 0, frame 712 is the first whose seeds give a pixel
    (1230) a first traversal draw of exactly 0.0 -- there, and nowhere else, the card commits and the base-colour image shows it; one frame on, no pixel does"""
    from tests import orc
    from vk_raytrace_amd import host_device as hd
    frame, pixels = io.first_zero_frame()
    assert (frame, list(pixels)) == (712, [1230])
    cfg = io.frames_config(kat, hd.eBaseColor)
    o = orc.Oracle()
    o.set_scene(cfg.scene)
    integral, _ = o.set_env(cfg.env)
    o.set_camera(cfg.camera)
    o.set_sunsky(cfg.sunsky)
    assert list(io.card_pixels(o.render(cfg.state(integral), 1, first_frame=frame), frame)) == [1230]
    assert o.stats()["alphaTests"] >= io.FRAME_SIZE ** 2                # every primary ray drew for the card
    assert len(io.card_pixels(o.render(cfg.state(integral), 1, first_frame=frame + 1), frame + 1)) == 0
    o.close()

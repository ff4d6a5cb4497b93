"""GPU tests at the edges the parity suite's scenes never reach: traversal stacks deeper than the LDS part (the private spill array) and deeper
than the whole stack (the overflow contract), maxDepth outside 3..10, and image shards of more ranks than two, down to ranks that own no tile.

The deep scenes come from synth.deep_chain; tests/test_trace_host.py proves on the CPU, with the product's own traversal source and builder,
that the spill scene drives walks past stack level STACK_LDS = 24 (and not past 64) and that the overflow scene goes past 64.  Every image is
compared with the CPU oracle bit for bit.
"""
import os

import numpy as np
import pytest

from tests import orc
from tests.common import Config, render_hip, render_oracle
from tests.test_gpu_parity import _render_in_subprocess, assert_identical
from vk_raytrace_amd import capi, host_device as hd, shard, synth

pytestmark = pytest.mark.gpu
W, H = 64, 48


@pytest.fixture(scope="module")
def env_small():
    return synth.procedural_sky(256, 128)


def spill_cfg(env, **kw):
    return Config(synth.deep_chain(synth.DEEP_SPILL_LEVELS), env, W, H, **kw)


# ---- 1. spill scene: every traversal kernel walks levels 25..64, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL])
def test_spill_scene_first_hit_aovs(env_small, accel):
    for mode in (hd.eNormal, hd.eTexcoord):
        cfg = spill_cfg(env_small, debug=mode)
        h = render_hip(cfg, 1, accel=accel)
        assert h[..., :3].any()
        assert np.array_equal(h, render_oracle(cfg, 1)), (accel, mode)


def test_spill_scene_path_traced_through_every_traversal_kernel():
    """default (packet + trace machine), the lock-step walks of k_tail, the staged chain, the fused kernels, the exact fallbacks (MASK /
    BLEND slivers in the deep region), the builders, the compact nodes; flat, two-level, two-level with one BLAS per prim-mesh.  Each
    renders in a fresh process with PT_TUNE (the launch-policy knobs are read at pt_create); an overflow would fail its pt_read_accum."""
    cfg = Config(synth.deep_chain(synth.DEEP_SPILL_LEVELS), synth.procedural_sky(128, 64), 64, 48, depth=5, max_samples=2)   # the "spill" scene of the helper
    ref = render_oracle(cfg, 3)
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0
    for tune in ("", "tail=0", "tail=1000000000", "packetClosest=0", "cnodes=0", "fuse=0", "fuse=2", "build=lbvh", "build=ploc", "build=sah",
                 "accel=two", "accel=two,tail=0", "accel=two,tail=1000000000", "accel=two,packetClosest=0", "accel=two,cnodes=0", "accel=two,fuse=0",
                 "accel=two,fuse=2", "accel=two,build=lbvh", "accel=two,build=sah", "accel=two,mergeSingles=0", "accel=two,mergeSingles=0,tail=0",
                 "accel=two,mergeSingles=0,tail=1000000000", "arena=0", "accel=two,arena=0"):
        assert_identical(_render_in_subprocess(tune, frames=3, max_samples=2, scene="spill"), ref, f"PT_TUNE={tune!r}")


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL])
def test_spill_scene_counters_and_picker(env_small, accel):
    cfg = spill_cfg(env_small, depth=6)
    (h, r), (o, oo) = render_hip(cfg, 2, return_obj=True, accel=accel), render_oracle(cfg, 2, return_obj=True)
    assert_identical(h, o, "spill scene, depth 6")
    hs, os_ = r.stats(), oo.stats()   # pt_get_stats: PT_OK (no overflow)
    for k in ("samples", "closestRays", "shadowRays", "shadedHits", "misses", "alphaTests", "neeLookups"):
        assert hs[k] == os_[k], (k, hs[k], os_[k])
    assert hs["alphaTests"] > 0
    oo.close()
    # pt_pick through the deep region: every triangle counts for the picker, as for the oracle's probe with any-hit off
    probe = orc.Oracle()
    probe.use_any_hit(False)
    probe.set_scene(cfg.scene)
    hits = 0
    for (x, y) in [(0.5, 0.5), (0.52, 0.47), (0.45, 0.55), (0.6, 0.5), (0.5, 0.62), (0.38, 0.41), (0.58, 0.36)]:
        p = r.pick(x, y, cfg.camera)
        org = np.array([list(p.worldRayOrigin)], np.float32); d = np.array([list(p.worldRayDirection)], np.float32)
        t, node, prim, uv, _ = probe.trace_closest(org, d)
        if node[0] < 0:
            assert p.instanceID == 0xFFFFFFFF
            continue
        hits += 1
        assert (p.instanceID, p.primitiveID) == (int(node[0]), int(prim[0])), (x, y)
        assert p.hitT == t[0] and p.baryCoord[1] == uv[0, 0] and p.baryCoord[2] == uv[0, 1]
    assert hits >= 3
    probe.close()
    r.destroy()


# ---- 2. overflow scene: reported by every call that hands out results, until the counter is cleared -------------------------------------
def _expect_overflow(fn):
    with pytest.raises(capi.PtError) as e:
        fn()
    assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value), str(e.value)


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL])
def test_overflow_is_reported_everywhere_and_cleared(env_small, accel):
    from vk_raytrace_amd.renderer import HipRenderer
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), env_small, 32, 24, depth=2)
    shallow = Config(synth.feature_box(tex_size=32), env_small, 32, 24, depth=4)
    tm = hd.default_tonemapper()
    r = HipRenderer(); r.setup(0); r.set_accel_mode(accel)
    r.set_scene(deep.scene); integral, _ = r.set_env(deep.env); r.set_camera(deep.camera); r.set_sunsky(deep.sunsky); r.create((32, 24))

    def frame(cfg, f=0):
        st = cfg.state(integral); st.frame = f
        r.setPushContants(st); r.run()

    # the display loop finds out first: pt_tonemap_begin knows nothing yet, pt_tonemap_end reads the counter the pass copied
    frame(deep)
    r.tonemap_begin(tm)
    _expect_overflow(r.tonemap_end)
    # ... and from then on every call that hands out results says so
    _expect_overflow(r.synchronize)
    _expect_overflow(r.read_accum)
    _expect_overflow(lambda: r.tonemap(tm))
    _expect_overflow(lambda: r.tonemap_begin(tm))
    assert r.tonemap_pending() == 0
    _expect_overflow(lambda: r.pick(0.5, 0.5, deep.camera))
    _expect_overflow(r.local_shard)
    _expect_overflow(r.stats)
    _expect_overflow(r.synchronize)   # still: the state is sticky
    # a fresh render, first looked at through pt_synchronize / pt_pick / pt_local_shard
    r.reset_stats()
    r.synchronize(); r.read_accum(); r.stats()
    for first in (r.synchronize, lambda: r.pick(0.5, 0.5, deep.camera), r.local_shard):
        frame(deep)
        _expect_overflow(first)
        _expect_overflow(r.read_accum)
        r.reset_stats()
    # pt_reset_stats alone clears it
    frame(deep)
    _expect_overflow(r.synchronize)
    r.reset_stats()
    r.synchronize(); r.read_accum(); r.tonemap(tm); r.stats(); r.local_shard()
    # a new, shallow scene after an overflow renders with PT_OK and equals the oracle (pt_build_accel clears the counter)
    frame(deep)
    _expect_overflow(r.synchronize)
    r.set_scene(shallow.scene); r.set_camera(shallow.camera)
    for f in range(2):
        frame(shallow, f)
    r.synchronize()
    r.tonemap_begin(tm); r.tonemap_end()
    assert_identical(r.read_accum(), render_oracle(shallow, 2), "shallow scene after an overflowing one")
    r.stats()
    # images still pending when the overflow is cleared: the clear covers them, and the display loop goes on with PT_OK
    for clear in ("pt_reset_stats", "pt_build_accel"):
        r.set_scene(deep.scene); r.set_camera(deep.camera)
        frame(deep)
        r.tonemap_begin(tm)
        frame(deep, 1)
        r.tonemap_begin(tm)
        assert r.tonemap_pending() == 2
        _expect_overflow(r.tonemap_end)
        if clear == "pt_reset_stats":
            r.reset_stats()
            r.tonemap_end()              # the stale image of the deep scene, taken after the clear
            r.tonemap_begin(tm); r.tonemap_end()
            r.set_scene(shallow.scene)
        else:
            r.set_scene(shallow.scene)
            r.tonemap_end()
        r.set_camera(shallow.camera)
        for f in range(2):
            frame(shallow, f)
            r.tonemap_begin(tm)
            r.tonemap_end()
        r.synchronize()
        assert_identical(r.read_accum(), render_oracle(shallow, 2), f"shallow scene after a clear by {clear} with images pending")
        r.stats()
    r.destroy()


# ---- 3. maxDepth outside 3..10 ---------------------------------------------------------------------------------------------------------
def test_max_depth_extremes(env_small):
    room = synth.bright_room()
    imgs = {}
    old = os.environ.get("PT_TUNE")
    for tune in ("tail=0", "tail=65536"):
        os.environ["PT_TUNE"] = tune
        try:
            for depth in (0, 1, 2, 11, 64, 256):
                for ms in (1, 3):
                    cfg = Config(room, env_small, 40, 30, depth=depth, max_samples=ms)
                    h = render_hip(cfg, 2)
                    assert_identical(h, render_oracle(cfg, 2), f"maxDepth {depth}, maxSamples {ms}, {tune}")
                    imgs[(tune, depth, ms)] = h
            for mode in (hd.eRadiance, hd.eWeight, hd.eRayDir):   # the last bounce is the first
                cfg = Config(room, env_small, 40, 30, depth=1, debug=mode)
                assert_identical(render_hip(cfg, 1), render_oracle(cfg, 1), f"maxDepth 1, debug mode {mode}, {tune}")
        finally:
            if old is None:
                os.environ.pop("PT_TUNE", None)
            else:
                os.environ["PT_TUNE"] = old
    for ms in (1, 3):
        assert not np.array_equal(imgs[("tail=0", 64, ms)], imgs[("tail=0", 256, ms)])   # paths outlive 64 bounces: the long tail ran
        assert not np.array_equal(imgs[("tail=0", 11, ms)], imgs[("tail=0", 64, ms)])
        assert not imgs[("tail=0", 0, ms)][..., :3].any() and imgs[("tail=0", 1, ms)][..., :3].max() > 0   # depth 0: no bounce, nothing gathered
        assert np.isfinite(imgs[("tail=0", 256, ms)]).all()


def test_max_depth_out_of_range_is_invalid(env_small):
    cfg = Config(synth.bright_room(), env_small, 16, 16, depth=4)
    _, r = render_hip(cfg, 1, return_obj=True)
    for depth in (257, -1):
        st = cfg.state(r.env_integral); st.maxDepth = depth
        r.setPushContants(st)
        with pytest.raises(capi.PtError) as e:
            r.run()
        assert e.value.code == capi.PT_ERR_INVALID
    r.destroy()


# ---- 4. shards: more ranks than two, ragged images, ranks without tiles -------------------------------------------------------------------
@pytest.mark.parametrize("width,height,nranks", [(100, 37, 3), (100, 37, 5), (100, 37, 8), (64, 64, 8)])
def test_shards_equal_the_one_rank_image(env_small, width, height, nranks):
    cfg = Config(synth.feature_box(tex_size=32), env_small, width, height, depth=4)
    for accel in (capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL):
        full = render_hip(cfg, 2, accel=accel)
        shards = []
        for rank in range(nranks):
            img, r = render_hip(cfg, 2, shard=(rank, nranks), return_obj=True, accel=accel)
            ids = shard.local_pixel_ids(width, height, rank, nranks)
            flat_img, flat_full = img.reshape(-1, 4), full.reshape(-1, 4)
            assert np.array_equal(flat_img[ids].view(np.uint32), flat_full[ids].view(np.uint32)), (rank, nranks, accel)
            others = np.ones(width * height, bool); others[ids] = False
            assert not flat_img[others].any(), (rank, nranks, accel)
            ptr, nbytes, nloc, nmax = r.local_shard()
            assert nloc == len(shard.tiles_of_rank(width, height, rank, nranks)) and nmax == shard.max_tiles_per_rank(width, height, nranks)
            # a checkpoint restored into a shard keeps the rank's own pixels only
            r.write_accum(np.ones((height, width, 4), np.float32))
            back = r.read_accum().reshape(-1, 4)
            assert (back[ids] == 1).all() and not back[others].any(), (rank, nranks, accel)
            if nloc == 0:   # owns no tile: every call succeeds and hands out nothing but zeros
                assert not img.any()
                tm = hd.default_tonemapper()
                want = orc.tonemap(tm, np.zeros((height, width, 4), np.float32))
                r.synchronize()
                assert np.array_equal(r.tonemap(tm), want)
                r.tonemap_begin(tm)
                assert np.array_equal(r.tonemap_end(), want)
                r.stats()
            shards.append(img)
            r.destroy()
        if nranks == 8:   # (4 tiles of 64 x 64, 8 tiles of 100 x 37 over 8 ranks)
            assert any(not shard.tiles_of_rank(width, height, k, nranks) for k in range(nranks))
        assembled = shard.assemble_rowmajor(shards, width, height)
        assert np.array_equal(assembled.view(np.uint32), full.view(np.uint32)), (nranks, accel)

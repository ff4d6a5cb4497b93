"""The chained guide pass on the device (pt_render_guides_chain / pt_read_guide_chain through the C ABI) against the host build of
the same header (tests/chain_host.py), which tests/test_chain_host.py holds to the first-hit pass, to the query host build and to a float32 restatement:
device == host bit for bit on every pixel of the three planes and the link plane, on the flat structure with and without the per-slot shading lines and on
the two-level one; identity with pt_render_guides; the walks against pt_trace_rays; no side effects on a frame sequence, sharded too; the consumers of
the display path on chain planes against their host builds; refusals and masks."""
import ctypes as C

import numpy as np
import pytest

from tests import albedo_host as ah, chain_host as ch, guides_host, svgf_host as sh, temporal_host as th
from tests import test_chain_host as host
from tests import test_guides_host as ghost
from tests.common import Config
from tests.host_harness import NONE, ill_conditioned
from tests.test_guides_gpu import ENV, open_renderer
from tests.test_query_host import CANDIDATES, CLOSEST, host_query, make_rays, world_index
from vk_raytrace_amd import capi, host_device as hd, synth

pytestmark = pytest.mark.gpu
SIZES, APERTURES, MISS_DEPTH, bits, ROOM = host.SIZES, host.APERTURES, host.MISS_DEPTH, host.bits, host.ROOM
LINKS = (0, 1, 2, 8)
DIFFER_CAP = 3       # pixels of an image that may differ from the host build, each with its proof (the rule of tests/test_paths_gpu.py)
STRUCTURES = [("flat", capi.PT_ACCEL_FLAT, None), ("flat, shadeTris=0", capi.PT_ACCEL_FLAT, "shadeTris=0"), ("two-level", capi.PT_ACCEL_TWO_LEVEL, None)]


def capture(r, p, planes=7, miss_depth=MISS_DEPTH):
    r.capture_guides_chain(p, planes, miss_depth)
    return r.read_guides(planes), r.read_guide_chain()


def proven_differences(r, c, two, w, h, p, got, want, what):
    """Pixels that differ from the host build's.  Each must come with the proof: along one of the pixel's link records (the host's) the candidate lists of
    the device's tree and of the host harness's differ, and fp32's verdict on one of the two triangles at the first differing position is an artefact
    (host_harness.ill_conditioned)."""
    diff = np.zeros((h, w), bool)
    for j in range(3):
        diff |= (bits(got[0][j]) != bits(want[0][j])).any(-1)
    diff |= got[1] != want[1]
    bad = np.nonzero(diff.ravel())[0]
    assert len(bad) <= DIFFER_CAP, f"{what}: {len(bad)} pixels differ, first (y, x) {np.argwhere(diff)[:4].tolist()}"
    if len(bad):
        rec, cnt = ch.links(c.traced, two, w, h, p, pixels=bad, miss_depth=MISS_DEPTH)
    for i, px in enumerate(bad):
        for k in range(int(cnt[i])):
            one = make_rays(rec[i, k]["org"], rec[i, k]["dir"])
            dc, hc = r.trace_ray_records(CANDIDATES, one, 16)[0], host_query(c.traced, two, CANDIDATES, one, hits_per_ray=16)[0]
            dw, hw = world_index(c.scene, dc), world_index(c.scene, hc)
            at = np.nonzero((dw != hw) | (bits(dc["t"]) != bits(hc["t"])))[0]
            if len(at):
                a = int(at[0])
                o, d = one["origin"][0], one["direction"][0]
                assert any(x != NONE and ill_conditioned(c.traced.world_tri(x), o, d, tx) for x, tx in ((dw[a], dc["t"][a]), (hw[a], hc["t"][a]))), \
                    f"{what}: pixel {px}: a well-conditioned candidate differs at position {a}: device {dw} {dc['t']} vs host {hw} {hc['t']}"
                break
        else:
            raise AssertionError(f"{what}: pixel {px} differs although both trees report the same candidates along its chain")
    return len(bad)


# ---- 1. device against the host build -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", STRUCTURES, ids=[s[0] for s in STRUCTURES])
@pytest.mark.parametrize("name", (ROOM, "fuzz1"))
def test_device_equals_the_host_build_bit_for_bit(name, structure):
    """both sizes, pinhole and aperture, maxLinks 0, 1, 2 and 8; on fuzz1 every surface is followed besides (maxRoughness = 1, minMetallic = 0): walks after
    alpha draws.  Expected number of differing pixels: 0"""
    what, accel, tune = structure
    c = host.case(name)
    two = int(accel == capi.PT_ACCEL_TWO_LEVEL)
    sets = [ch.params(n) for n in LINKS] + ([ch.params(2, 1.0, 0.0, 0.0)] if name == "fuzz1" else [])
    r = open_renderer(c.scene, accel=accel, tune=tune)
    seen = followed = 0
    try:
        for (w, h) in SIZES:
            r.create((w, h))
            for ap in APERTURES:
                r.set_camera(c.set_camera(w, h, ap))
                for p in sets:
                    want = ch.chain(c.traced, two, w, h, p, 7, MISS_DEPTH)
                    got = capture(r, p)
                    seen += proven_differences(r, c, two, w, h, p, got, want, f"{name} {what} {w}x{h} aperture {ap} maxLinks {p.maxLinks}")
                    followed += int((want[1] & 255).sum())
    finally:
        r.destroy()
    print(f"{name} {what}: {seen} pixels differ from the host build (all through ill-conditioned candidates)")
    assert followed > 1000


# ---- 2. identity with the first-hit pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", STRUCTURES, ids=[s[0] for s in STRUCTURES])
def test_without_links_the_planes_are_pt_render_guides(structure):
    what, accel, tune = structure
    c = host.case(ROOM)
    r = open_renderer(c.scene, accel=accel, tune=tune)
    try:
        for (w, h) in SIZES:
            r.create((w, h))
            for ap in APERTURES:
                r.set_camera(c.set_camera(w, h, ap))
                r.capture_guides(7, MISS_DEPTH)
                want = r.read_guides()
                for p in (ch.params(0), ch.params(8, min_metallic=2.0, min_transmission=2.0)):
                    got, links = capture(r, p)
                    host.assert_planes_equal(got, want, f"{what} {w}x{h} aperture {ap}")
                    assert (links & 255 == 0).all() and np.array_equal(links >> 8 == ch.END_MISS, want[2][..., 0] == np.float32(MISS_DEPTH))
    finally:
        r.destroy()


# ---- 3. the walks against pt_trace_rays -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
def test_the_length_of_one_link_is_two_closest_hit_queries(accel):
    """plane 2 on the pixels of one link == t0 + t1 of two pt_trace_rays(PT_RAYS_CLOSEST) calls on the host build's link records"""
    c = host.case(ROOM)
    w, h = SIZES[0]
    two = int(accel == capi.PT_ACCEL_TWO_LEVEL)
    p = ch.params(8)
    cam = c.set_camera(w, h, 0.0)
    (_, links), (rec, cnt) = ch.chain(c.traced, two, w, h, p, 7, MISS_DEPTH), ch.links(c.traced, two, w, h, p, miss_depth=MISS_DEPTH)
    one = (links.ravel() == 1) & (cnt == 2)
    assert one.sum() > 500
    r = open_renderer(c.scene, (w, h), accel=accel)
    try:
        r.set_camera(cam)
        t = [r.trace_rays(CLOSEST, rec[one, k]["org"], rec[one, k]["dir"], seeds=rec[one, k]["seed"])["t"] for k in (0, 1)]
        planes, dev_links = capture(r, p, capi.PT_GUIDES_DEPTH)
        same = bits(planes[2][..., 0].ravel()[one]) == bits(t[0] + t[1])
        assert same.sum() >= one.sum() - DIFFER_CAP and (dev_links.ravel()[one] == 1).sum() >= one.sum() - DIFFER_CAP
    finally:
        r.destroy()


# ---- 4. no side effects -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shard", [None, (1, 2)], ids=["whole", "rank 1 of 2"])
def test_a_frame_sequence_with_chain_passes_in_between_continues_bit_for_bit(shard):
    """six frames with pt_render_guides_chain after frames 0, 2 and 3 and no synchronisation in between: accumulation image and counters of the
    uninterrupted run; on a sharded context too, where the pass still renders the whole image"""
    c = host.case(ROOM)
    w, h = 64, 48
    cfg = Config(c.scene, ENV, w, h)
    p = ch.params(8)
    results = []
    for interrupt in (False, True):
        r = open_renderer(cfg.scene, (w, h), shard=shard)
        try:
            r.set_camera(cfg.camera)
            st = cfg.state(r.env_integral)
            r.reset_stats()
            for f in range(6):
                st.frame = f
                r.setPushContants(st)
                r.run()
                if interrupt and f in (0, 2, 3):
                    r.capture_guides_chain(p, 7, MISS_DEPTH)
            img = r.read_accum()
            stats = {k: v for k, v in r.stats().items() if not k.startswith("ms")}
            if interrupt:
                planes, links = r.read_guides(), r.read_guide_chain()
                guides_host.set_camera(c.traced, cfg.camera)
                want = ch.chain(c.traced, 0, w, h, p, 7, MISS_DEPTH)
                assert proven_differences(r, c, 0, w, h, p, (planes, links), want, f"shard {shard}") <= DIFFER_CAP
                assert (links & 255).max() >= 2
            st.frame = 6
            r.setPushContants(st)
            r.run()
            results.append((img, stats, r.read_accum()))
        finally:
            r.destroy()
    (img_a, stats_a, next_a), (img_b, stats_b, next_b) = results
    assert np.array_equal(bits(img_a), bits(img_b)) and stats_a == stats_b and stats_a["samples"] > 0
    assert np.array_equal(bits(next_a), bits(next_b))


# ---- 5. the consumers of the display path on chain planes -------------------------------------------------------------------------------------------------------
def test_the_display_stages_on_chain_planes_equal_their_host_builds():
    """pt_temporal_accumulate (plain, and with pt_temporal_demodulate(1) and moments), pt_svgf_history and pt_tonemap_svgf on the planes the chained pass
    left in the context, over a camera strafe, against the host builds of the stages fed the planes read back: the existing device == host relation on the
    new inputs"""
    c = host.case(ROOM)
    w, h = SIZES[1]
    cam0 = c.scene.camera
    cams = [(cam0.eye, cam0.center), host.chain_scenes.strafed(cam0)]
    p = ch.params(8)
    rng = np.random.default_rng(11)
    r = open_renderer(c.scene, (w, h))
    old = (cam0.eye, cam0.center)
    try:
        for demodulate in (False, True):
            r.temporal_demodulate(demodulate)
            r.track_moments(demodulate)
            r.temporal_reset()
            hist = None
            for k, (eye, center) in enumerate(cams):
                cam0.eye, cam0.center = eye, center
                cam = ghost.camera_for(c.scene, w, h, 0.0)
                w2c = capi.camera_world_to_clip(cam0, w / h)
                r.set_camera(cam)
                planes, links = capture(r, p, 7, 100.0)
                colour = (planes[0] * np.float32(2.0) + rng.uniform(0, 0.05, (h, w, 4)).astype(np.float32)).astype(np.float32)
                r.write_accum(colour)
                tp = r.temporal_params(w2c, 0.05, 0.05, 32.0)
                got = r.temporal_accumulate(tp)
                if demodulate:
                    rc, hist = ah.temporal(colour, planes[0], planes[1], planes[2], cam.viewInverse, cam.projInverse, tp, hist, moments=True)
                else:
                    rc, hist = th.temporal(colour, planes[1], planes[2], cam.viewInverse, cam.projInverse, tp, hist)
                assert rc == 0
                hc, hn = r.read_temporal_history()
                assert np.array_equal(bits(got), bits(hist.colour)) and np.array_equal(bits(hc), bits(hist.colour)) and np.array_equal(bits(hn), bits(hist.length)), (demodulate, k)
            assert (hist.length[(links & 255) == 1] > 1).mean() > 0.5      # the reflection kept its history across the strafe
            if demodulate:
                sp = sh.params(3, sigma_guide=(0.5, 0.3, 0.5), min_temporal=1.5)
                rc, img, var = ah.svgf_history(hist, planes, sp)
                assert rc == 0
                dc, dv = r.svgf_history(sp)
                assert np.array_equal(bits(dc), bits(img)) and np.array_equal(bits(dv), bits(var))
                tm = hd.default_tonemapper()
                shown = r.tonemap_svgf(sp, tm)
                r.write_accum(dc)
                assert np.array_equal(shown, r.tonemap(tm))
    finally:
        cam0.eye, cam0.center = old
        r.temporal_demodulate(False)
        r.track_moments(False)
        r.destroy()


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_plane_masks_and_resize():
    c = host.case(ROOM)
    w, h = SIZES[1]
    p = ch.params(8)
    r = open_renderer(c.scene, (w, h))
    try:
        r.set_camera(c.set_camera(w, h, 0.0))
        with pytest.raises(capi.PtError) as e:
            r.read_guide_chain()
        assert e.value.code == capi.PT_ERR_STATE and "pt_render_guides_chain" in str(e.value)
        full, links = capture(r, p)
        mine = np.full((h, w, 4), 0.375, np.float32)
        # an installed plane outside the mask survives, one inside it is replaced, an unset one outside it stays unset; the link plane is always written
        r.set_denoise_guides(mine, mine, None)
        r.capture_guides_chain(ch.params(0), capi.PT_GUIDES_NORMAL, MISS_DEPTH)
        got = r.read_guides(capi.PT_GUIDES_BASECOLOR | capi.PT_GUIDES_NORMAL)
        assert np.array_equal(got[0], mine) and got[2] is None and (r.read_guide_chain() & 255 == 0).all()
        r.capture_guides_chain(p, capi.PT_GUIDES_NORMAL, MISS_DEPTH)
        got = r.read_guides(capi.PT_GUIDES_BASECOLOR | capi.PT_GUIDES_NORMAL)
        assert np.array_equal(got[0], mine) and np.array_equal(bits(got[1]), bits(full[1])) and np.array_equal(r.read_guide_chain(), links)
        with pytest.raises(capi.PtError) as e:
            r.read_guides(capi.PT_GUIDES_DEPTH)
        assert e.value.code == capi.PT_ERR_STATE
        # a resize to the same size keeps the link plane, one to another size drops it
        r.create((w, h))
        assert np.array_equal(r.read_guide_chain(), links)
        r.create((w + 3, h))
        with pytest.raises(capi.PtError) as e:
            r.read_guide_chain()
        assert e.value.code == capi.PT_ERR_STATE
        r.set_camera(c.set_camera(w + 3, h, 0.0))
        r.capture_guides_chain(p, capi.PT_GUIDES_BASECOLOR)
        assert r.read_guide_chain().shape == (h, w + 3)
    finally:
        r.destroy()


def test_refusals():
    L = capi.lib()
    c = host.case(ROOM)
    w, h = SIZES[1]
    good = ch.params(4)
    links = np.zeros((h, w), np.uint32)
    # before a scene / an acceleration structure, before a camera, before a size
    r = open_renderer(None, (w, h))
    try:
        assert L.pt_render_guides_chain(r._ctx, C.byref(good), 7, 1.0) == capi.PT_ERR_STATE and b"pt_build_accel" in L.pt_last_error(r._ctx)
        r.set_scene(c.scene)
        assert L.pt_render_guides_chain(r._ctx, C.byref(good), 7, 1.0) == capi.PT_ERR_STATE and b"pt_set_camera" in L.pt_last_error(r._ctx)
    finally:
        r.destroy()
    r = open_renderer(c.scene)
    try:
        r.set_camera(ghost.camera_for(c.scene, w, h, 0.0))
        assert L.pt_render_guides_chain(r._ctx, C.byref(good), 7, 1.0) == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        assert L.pt_read_guide_chain(r._ctx, links.ctypes.data) == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        r.create((w, h))
        assert L.pt_read_guide_chain(r._ctx, links.ctypes.data) == capi.PT_ERR_STATE and ch.need_plane(False)[1].encode() in L.pt_last_error(r._ctx)
        assert L.pt_read_guide_chain(r._ctx, None) == capi.PT_ERR_INVALID
        assert L.pt_render_guides_chain(None, C.byref(good), 7, 1.0) == capi.PT_ERR_INVALID and L.pt_read_guide_chain(None, links.ctypes.data) == capi.PT_ERR_INVALID
        before = capture(r, good)
        # arguments: nothing is launched, the planes stay what they were; the chain parameters' refusals carry chain_constants' text
        for planes, miss in ((0, 1.0), (8, 1.0), (15, 1.0), (7, float("nan")), (7, float("inf")), (7, float("-inf"))):
            assert L.pt_render_guides_chain(r._ctx, C.byref(good), planes, miss) == capi.PT_ERR_INVALID, (planes, miss)
        bad = [None, ch.params(9), ch.params(4, max_roughness=-1.0), ch.params(4, max_roughness=float("nan")), ch.params(4, min_metallic=float("inf")),
               ch.params(4, min_transmission=-0.5), ch.params(4, flags=2)]
        texts = set()
        for p in bad:
            rc, why = ch.constants(p)
            assert L.pt_render_guides_chain(r._ctx, None if p is None else C.byref(p), 7, 1.0) == capi.PT_ERR_INVALID == rc
            assert why and why.encode() in L.pt_last_error(r._ctx) and b"pt_render_guides_chain" in L.pt_last_error(r._ctx), why
            texts.add(why)
        assert len(texts) == 6
        after = r.read_guides(), r.read_guide_chain()
        host.assert_planes_equal(after[0], before[0], "after refused calls")
        assert np.array_equal(after[1], before[1])
        ms = C.c_float(-1.0)
        assert L.pt_debug_guides_chain_time(r._ctx, C.byref(good), 7, MISS_DEPTH, 2, C.byref(ms)) == capi.PT_OK and ms.value > 0
        assert L.pt_debug_guides_chain_time(r._ctx, C.byref(good), 7, MISS_DEPTH, 0, C.byref(ms)) == capi.PT_ERR_INVALID
        assert L.pt_debug_guides_chain_time(r._ctx, C.byref(bad[1]), 7, MISS_DEPTH, 2, C.byref(ms)) == capi.PT_ERR_INVALID
    finally:
        r.destroy()


def test_an_overflow_of_its_walks_is_reported_by_the_next_synchronising_call():
    """the overflow scene of tests/test_gpu_edges.py: the pass itself returns PT_OK (asynchronous), pt_read_guide_chain reports the overflow"""
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), ENV, 32, 24, depth=2)
    r = open_renderer(deep.scene, (32, 24))
    try:
        r.set_camera(deep.camera)
        r.capture_guides_chain(ch.params(8))
        for fn in (r.read_guide_chain, r.synchronize):
            with pytest.raises(capi.PtError) as e:
                fn()
            assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value)
        r.reset_stats()
        r.synchronize()
    finally:
        r.destroy()

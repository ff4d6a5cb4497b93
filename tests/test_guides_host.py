"""The guide pass on the CPU: vk_raytrace_amd/csrc/pt_guides.h (guide_pixel<TWO>, what pt_render_guides runs per lane) compiled for the host by
tests/cpp/guides_host.cpp and held, pixel by pixel and bit for bit, to the oracle.

Claim under test ("Guide pass"): for every pixel, plane 0 and plane 1 are what the oracle accumulates in frame 0 under
debugging_mode = eBaseColor / eNormal (maxSamples 1, maxDepth 2, a firefly threshold that never engages: the guide pass does not clamp), alpha
included; plane 2 holds in .x the `t` of the oracle's closest-hit trace of the very ray the colour and normal planes were shaded from -- the frame-0
camera ray with its depth-of-field draws, walked with the seed those draws leave behind -- or miss_depth, and zero in .yzw; and the walk leaves the RNG
state the oracle's walk leaves.  On the flat and on the two-level structure, at a size that is a multiple of the 8 x 8 pixel block and at one that is not,
with a pinhole and with an aperture (the depth-of-field draws precede the alpha draws: this pins the order), on the configurations of the whole-frame
host tests (tests/test_trace_host.py) and on the alpha scenes (MASK / BLEND materials, opacity maps, normal maps, vertex colours, mirrored instances).

The cameras are fixed so that every image shows hits and misses, and the alpha scenes walk the stochastic-alpha path; the tests assert that too
(conditions on the inputs, established on the oracle alone).  tests/test_guides_gpu.py holds the device to this host build."""
import functools

import numpy as np
import pytest

from tests import guides_host, orc
from tests.host_harness import OPAQUE, NOCULL, Traced, TracedScene
from vk_raytrace_amd import capi, host_device as hd, synth

SIZES = [(96, 64), (45, 37)]        # whole 8 x 8 blocks; partial blocks on both edges
APERTURES = [0.0, 0.05]
MISS_DEPTH = 12345.0
ALPHA_SCENES = ("fuzz0", "fuzz1", "fuzz5", "sponza-like")


def _look(scene, eye, center, fov=None):
    scene.camera.eye, scene.camera.center = eye, center
    if fov is not None:
        scene.camera.fov = fov
    return scene


# name -> scene with the camera of the test.  The first five are the scenes of the whole-frame host tests (tests/test_trace_host.py), the rest the
# alpha scenes (host_harness.alpha_scenes).  Where a scene's own camera shows only hits (interiors) or too few, a camera is set here: every image
# must hold both hits and misses (test_the_inputs_exercise_hits_misses_and_alpha_draws).
SCENES = {
    "feature-box": lambda: synth.feature_box(tex_size=32),
    "fuzz2": lambda: synth.fuzz_scene(2),
    "fuzz4": lambda: synth.fuzz_scene(4),
    "c3-stand-in": lambda: _look(_c3(), (-10.4, 2.2, 0.6), (12.0, 14.0, -0.4)),        # its own camera looks along the atrium: 96 % hits; this one sees the sky above it
    "deep-chain": lambda: synth.deep_chain(synth.DEEP_SPILL_LEVELS),
    "fuzz0": lambda: synth.fuzz_scene(0),
    "fuzz1": lambda: synth.fuzz_scene(1),
    "fuzz5": lambda: synth.fuzz_scene(5),
    "sponza-like": lambda: _look(synth.sponza_like(target_tris=12000, tex_size=64), (-10.4, 2.2, 0.6), (12.0, 14.0, -0.4)),
}


def _c3():
    from vk_raytrace_amd import workloads
    return workloads.c3_sponza(160, 90, 4, tex_size=64, env_w=256).scene


def camera_for(scene, width, height, aperture):
    cam = capi.camera_lookat(scene.camera, width / height, nb_lights=len(scene.lights))
    cam.aperture = aperture
    return cam


def guide_state(width, height, debug):
    st = hd.default_rtx_state()
    st.size[0], st.size[1] = width, height
    st.maxSamples, st.maxDepth, st.debugging_mode, st.fireflyClampThreshold = 1, 2, debug, 1e32
    return st


class Case:
    """one scene on the oracle and on the host harness; the oracle's answers per (size, aperture) are computed once and shared"""

    def __init__(self, name):
        self.name = name
        self.scene = SCENES[name]()
        if self.scene.vertices is None:
            self.scene.finalize(capi.pack_vertices)
        self.oracle = orc.Oracle()
        self.oracle.set_scene(self.scene)
        self.oracle.set_env(synth.procedural_sky(64, 32))
        self.oracle.set_sunsky(hd.default_sun_and_sky())
        self.traced = TracedScene(self.scene)
        self._ref = {}

    def set_camera(self, width, height, aperture):
        cam = camera_for(self.scene, width, height, aperture)
        self.oracle.set_camera(cam)
        guides_host.set_camera(self.traced, cam)
        return cam

    def reference(self, width, height, aperture):
        """(base colour image, normal image) of the oracle's frame 0"""
        key = (width, height, aperture)
        if key not in self._ref:
            self.set_camera(width, height, aperture)
            self._ref[key] = tuple(self.oracle.render(guide_state(width, height, mode), 1) for mode in (hd.eBaseColor, hd.eNormal))
            for img in self._ref[key]:
                img.setflags(write=False)
        return self._ref[key]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_depth(c, width, height, aperture):
    """the oracle's closest-hit trace of the host build's camera rays, started from the seed the camera leaves: (hit mask, t, seed after the walk,
    seed after the camera, seed after the host's walk)"""
    c.set_camera(width, height, aperture)
    org, dirs, s_cam, s_walk = guides_host.rays(c.traced, width, height)
    t, node, _, _, s_orc = c.oracle.trace_closest(org, dirs, s_cam)
    return node >= 0, t, s_orc, s_cam, s_walk


@pytest.mark.parametrize("name", list(SCENES))
def test_colour_and_normal_planes_are_the_oracles_first_hit_debug_frames(name):
    c = case(name)
    for (w, h) in SIZES:
        for ap in APERTURES:
            ref = c.reference(w, h, ap)
            c.set_camera(w, h, ap)
            for two in (0, 1):
                got = guides_host.guides(c.traced, two, w, h, capi.PT_GUIDES_BASECOLOR | capi.PT_GUIDES_NORMAL, MISS_DEPTH)
                for j, what in ((0, "base colour"), (1, "normal")):
                    same = (bits(got[j]) == bits(ref[j])).all(-1)
                    assert same.all(), f"{name} {w}x{h} aperture {ap} two={two}: {what} differs at {np.count_nonzero(~same)} pixels, first (y, x) {np.argwhere(~same)[:4].tolist()}"
                assert got[2] is None


@pytest.mark.parametrize("name", list(SCENES))
def test_depth_plane_is_the_oracles_closest_hit_of_the_same_ray(name):
    c = case(name)
    for (w, h) in SIZES:
        for ap in APERTURES:
            hit, t, s_orc, s_cam, s_walk = oracle_depth(c, w, h, ap)
            assert np.array_equal(s_walk, s_orc), f"{name} {w}x{h} aperture {ap}: the RNG state after the walk differs at {np.count_nonzero(s_walk != s_orc)} pixels"
            want = np.where(hit, t, np.float32(MISS_DEPTH)).astype(np.float32).reshape(h, w)
            for two in (0, 1):
                got = guides_host.guides(c.traced, two, w, h, capi.PT_GUIDES_DEPTH, MISS_DEPTH)
                assert got[0] is None and got[1] is None
                same = bits(got[2][..., 0]) == bits(want)
                assert same.all(), f"{name} {w}x{h} aperture {ap} two={two}: depth differs at {np.count_nonzero(~same)} pixels, first (y, x) {np.argwhere(~same)[:4].tolist()}"
                assert not bits(got[2][..., 1:]).any()
            # the mask of hits is the colour plane's: a miss is black there
            base, _ = c.reference(w, h, ap)
            assert not base[..., :3].reshape(-1, 3)[~hit].any()


def test_the_inputs_exercise_hits_misses_and_alpha_draws():
    """conditions on the inputs, from the oracle alone: every image holds between 10 % and 90 % of hits; over the alpha scenes at least 1 % of the
    pixels draw during the walk"""
    drew = total = 0
    for name in SCENES:
        c = case(name)
        for (w, h) in SIZES:
            for ap in APERTURES:
                hit, _, s_orc, s_cam, _ = oracle_depth(c, w, h, ap)
                assert 0.10 <= hit.mean() <= 0.90, f"{name} {w}x{h} aperture {ap}: {hit.mean():.3f} of the pixels hit"
                if name in ALPHA_SCENES:
                    drew += int(np.count_nonzero(s_orc != s_cam))
                    total += hit.size
    assert drew >= 0.01 * total, f"{drew} of {total} pixels of the alpha scenes draw"


def test_a_mask_of_one_plane_writes_only_that_plane():
    c = case("fuzz1")
    w, h = SIZES[1]
    c.set_camera(w, h, APERTURES[1])
    full = guides_host.guides(c.traced, 0, w, h, 7, MISS_DEPTH)
    sentinel = np.float32(-7.25)
    for j in range(3):
        into = [np.full((h, w, 4), sentinel, np.float32) for _ in range(3)]
        got = guides_host.guides(c.traced, 0, w, h, 1 << j, MISS_DEPTH, into=into)
        for k in range(3):
            if k == j:
                assert np.array_equal(bits(got[k]), bits(full[k])), (j, k)
            else:
                assert (got[k] == sentinel).all(), (j, k)


def test_without_any_hit_the_walk_makes_no_draw():
    """pt_use_any_hit(0) makes every instance opaque (the harness' build from instance flags): the seed after the walk is the seed after the camera,
    with an aperture too, although the same rays draw on the scene's own flags"""
    c = case("fuzz1")
    w, h = SIZES[0]
    opaque = Traced(c.scene, [OPAQUE | NOCULL] * len(c.scene.nodes))
    drew = 0
    for ap in APERTURES:
        cam = camera_for(c.scene, w, h, ap)
        guides_host.set_camera(opaque, cam)
        _, _, s_cam, s_walk = guides_host.rays(opaque, w, h)
        assert np.array_equal(s_cam, s_walk), ap
        guides_host.set_camera(c.traced, cam)
        org, dirs, s_cam2, s_walk2 = guides_host.rays(c.traced, w, h)
        assert np.array_equal(s_cam, s_cam2)
        drew += int(np.count_nonzero(s_cam2 != s_walk2))
    assert drew > 0
    opaque.close()

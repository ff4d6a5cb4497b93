"""pt_temporal_accumulate_moving on the device against the host build of the same header (tests/motion_host.py), which
tests/test_motion_model.py holds to the float64 model: device == host bit for bit on the returned image, the history colour, the length plane and, with
tracking on, the moments, over every move of the fixture as a three-call sequence on a three-node scene whose nodes pt_update_instances moves, hostile
instance planes and hostile node matrices; unchanged matrices give pt_temporal_accumulate; a rendered sequence in which a box slides along a wall; the
state machine."""
import ctypes as C

import numpy as np
import pytest

from tests import motion_host as mh, temporal_host as th
from tests import test_guides_gpu as gg
from tests import test_guides_host as ghost
from tests import test_motion_model as model
from tests.test_temporal_gpu import camera_words, rmse
from vk_raytrace_amd import capi, synth
from vk_raytrace_amd.renderer import HipRenderer
from vk_raytrace_amd.scene import Scene, translate

pytestmark = pytest.mark.gpu
mk, gen, bits = model.mk, model.gen, model.bits

# not multiples of the 32 x 8 block tile, one pixel, thinner than a tile in each direction
SIZES = [(70, 45), (45, 37), (1, 1), (3, 200), (129, 17)]


def three_node_scene():
    """three boxes, one node each: what the nodes show does not matter here (images, planes and the instance plane come through the setters), their
    world matrices do"""
    sc = Scene("motion_three_nodes")
    m = sc.add_material()
    for k in range(3):
        synth._add(sc, synth.box((0.5, 0.4, 0.3)), m, translate(1.5 * k, 0.0, 0.0))
    sc.finalize(capi.pack_vertices)
    return sc


def node_array(sc, worlds):
    nd = sc.node_array()
    for i, m in enumerate(worlds):
        nd[i]["worldMatrix"] = np.asarray(m, np.float32).T.reshape(16)
    return nd


def words_of(worlds):
    return np.stack([mh.instance_words(np.asarray(m, np.float32)) for m in worlds])


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    sc = three_node_scene()
    r.set_scene(sc)
    yield r, sc
    r.destroy()


def test_the_instance_words_are_the_products(dev):
    """tests/motion_host.py instance_words restates set_instance_transform (csrc/pt_scene_records.cpp): held to the product's own words here, through its
    export pt_debug_two_level_pad, on the matrices this module uses"""
    L = capi.lib()
    L.pt_debug_two_level_pad.restype = C.c_int
    L.pt_debug_two_level_pad.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    for m in [mk.box_world(move) for move in mk.MOVES] + HOSTILE_WORLDS:
        m32 = np.ascontiguousarray(np.asarray(m, np.float32).T.reshape(16))
        out = np.zeros(27, np.float32)
        assert L.pt_debug_two_level_pad(m32.ctypes.data, 1.0, out.ctypes.data) == 0
        assert np.array_equal(bits(out[:24]), bits(mh.instance_words(np.asarray(m, np.float32))))


def step_both(dev, hist, hist_words, worlds, colour, g1, g2, ids, view_inverse, proj_inverse, p, moments, what, static=False):
    """one call on the device and on the host build from the same inputs and the host's history (which the device's has equalled so far): the nodes get
    the matrices `worlds`; compares everything the device hands out; returns the host's new history and the words that go with it"""
    r, sc = dev
    r.update_instances(node_array(sc, worlds))
    r.write_accum(colour)
    r.set_denoise_guides(None, g1, g2)
    r.set_instance_plane(ids)
    r.set_camera(camera_words((view_inverse, proj_inverse)))
    got = r.temporal_accumulate(p) if static else r.temporal_accumulate_moving(p)
    hc, hn = r.read_temporal_history()
    cur_words = words_of(worlds)
    tab = None if hist is None else mh.table(hist_words, cur_words)
    if static:
        tab = None if tab is None else np.zeros_like(tab)       # (no record is `moved`: the static form)
    rc, want = mh.temporal_moving(colour, g1, g2, view_inverse, proj_inverse, p, ids, tab, hist, moments=moments)
    assert rc == 0
    pairs = [("returned image", got, want.colour), ("history colour", hc, want.colour), ("history length", hn, want.length)]
    if moments:
        pairs.append(("moments", r.read_temporal_moments(), want.moments))
    for name, a, b in pairs:
        diff = bits(a) != bits(b)
        assert not diff.any(), f"{what}: {name} differs from the host build at {int(diff.reshape(diff.shape[0], diff.shape[1], -1).any(-1).sum())} pixels"
    return want, cur_words


def identity_worlds(box=None):
    return [np.eye(4), np.eye(4), np.eye(4) if box is None else box]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_bit_for_bit(dev, size):
    """every move of the fixture as a three-call sequence -- a first call with the box where the history has it, update_instances and the move, a static
    call after it -- so that both buffer sets have been read and written and the table has been made from kept words twice; with the moments tracked on
    every other move, so that both kernels run"""
    r, _ = dev
    w, h = size
    r.create((w, h))
    for m, move in enumerate(mk.MOVES):
        moments = m % 2 == 0
        r.track_moments(moments)
        r.temporal_reset()
        inp = mk.case_inputs(size, move)
        H = inp["hist"]
        start = gen.moved("none", w / h)
        g1_0, g2_0 = H["guide"].copy(), np.zeros((h, w, 4), np.float32)
        g1_0[..., 3], g2_0[..., 0] = 1.0, H["guide"][..., 3]
        p0 = th.params(start["worldToClip"], gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY)
        label = f"{w}x{h} {move}" + (" with moments" if moments else "")
        hist, words = step_both(dev, None, None, identity_worlds(), H["colour"], g1_0, g2_0, H["ids"], start["viewInverse"], start["projInverse"], p0, moments, label + " call 1")
        p = model.tmodel.params_of(inp)
        args = (inp["g1"], inp["g2"], inp["ids"], inp["viewInverse"], inp["projInverse"], p, moments)
        hist, words = step_both(dev, hist, words, identity_worlds(inp["box"]), inp["colour"], *args, label + " call 2")
        again = gen.noisy_colour(w, h, np.random.default_rng(w + h))
        step_both(dev, hist, words, identity_worlds(inp["box"]), again, *args, label + " call 3")
    r.track_moments(False)


# matrices at the edge of what a scene holds: a translation beyond fp32's integer range (the point's own coordinates vanish in it), rows that are nearly
# parallel (determinant 1e-6: an inverse of 1e6), a tiny scale, a mirrored scale of six orders of magnitude between its axes
HOSTILE_WORLDS = [translate(3.0e7, -2.0e7, 1.0e7), np.array([[1, 1, 1, 0.5], [1, 1.001, 1, -2], [1, 1, 1.001, 7], [0, 0, 0, 1]], np.float64),
                  np.diag([3.0e-3, 2.0e-3, 5.0e-3, 1.0]), np.diag([-1.0e3, 2.0e-3, 4.0, 1.0]) + translate(1.0e4, 0.0, -3.0) - np.eye(4)]


@pytest.mark.parametrize("size", [(70, 45), (45, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hostile_planes_and_node_matrices(dev, size):
    """instance words that name no node -- numInstances, 0x7fffffff, NONE, random words -- give the static form at those pixels, on the device as on the
    host; node matrices at the edge of what pt_update_instances accepts give what the host build gives, non-finite points and normals included"""
    r, _ = dev
    w, h = size
    r.create((w, h))
    r.track_moments(False)
    inp = mk.case_inputs(size, "slide")
    H = inp["hist"]
    start = gen.moved("none", w / h)
    g1_0, g2_0 = H["guide"].copy(), np.zeros((h, w, 4), np.float32)
    g1_0[..., 3], g2_0[..., 0] = 1.0, H["guide"][..., 3]
    p0 = th.params(start["worldToClip"], gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY)
    p = model.tmodel.params_of(inp)
    rng = np.random.default_rng(w)
    ids, pick = model.hostile_ids(inp, rng)
    for k, world in enumerate([inp["box"]] + HOSTILE_WORLDS):
        r.temporal_reset()
        hist, words = step_both(dev, None, None, identity_worlds(), H["colour"], g1_0, g2_0, H["ids"], start["viewInverse"], start["projInverse"], p0, False, f"hostile {k} call 1")
        worlds = [np.eye(4), world if k % 2 else np.eye(4), world]
        got, words2 = step_both(dev, hist, words, worlds, inp["colour"], inp["g1"], inp["g2"], ids, inp["viewInverse"], inp["projInverse"], p, False, f"hostile {k} call 2")
        rc, static = th.temporal(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, hist)
        assert rc == 0 and model.same_pixels(got, static)[pick].all(), k
        step_both(dev, got, words2, worlds, inp["colour"], inp["g1"], inp["g2"], inp["ids"], inp["viewInverse"], inp["projInverse"], p, False, f"hostile {k} call 3")


def test_update_instances_with_unchanged_matrices_gives_pt_temporal_accumulate(dev):
    """the moving form after a pt_update_instances that changed no matrix equals pt_temporal_accumulate bit for bit: image, history, length and moments"""
    r, _ = dev
    size = (70, 45)
    w, h = size
    r.create(size)
    r.track_moments(True)
    inp = mk.case_inputs(size, "yaw")
    H = inp["hist"]
    start = gen.moved("none", w / h)
    g1_0, g2_0 = H["guide"].copy(), np.zeros((h, w, 4), np.float32)
    g1_0[..., 3], g2_0[..., 0] = 1.0, H["guide"][..., 3]
    p0 = th.params(start["worldToClip"], gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY)
    p = model.tmodel.params_of(inp)
    worlds = identity_worlds(inp["box"])
    results = []
    for static in (False, True):
        r.temporal_reset()
        hist, words = step_both(dev, None, None, worlds, H["colour"], g1_0, g2_0, H["ids"], start["viewInverse"], start["projInverse"], p0, True, "call 1", static=static)
        step_both(dev, hist, words, worlds, inp["colour"], inp["g1"], inp["g2"], inp["ids"], inp["viewInverse"], inp["projInverse"], p, True, "call 2", static=static)
        results.append((*r.read_temporal_history(), r.read_temporal_moments()))
    for a, b in zip(*results):
        assert np.array_equal(bits(a), bits(b))
    r.track_moments(False)


# ---- a rendered sequence ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
def test_a_box_sliding_along_the_wall(accel):
    """three rounds of update_instances, pt_render_instance_plane, frame 0 and accumulate on the opaque scene of tests/test_guides_gpu.py, its second box
    moved along the wall by a fifth of its width per round, on two contexts fed the same calls: one accumulates with the moving form, the other with
    pt_temporal_accumulate.  The host build, fed what was read back, reproduces every round of both.  On the pixels of the moved box the moving form ends with
    a strictly larger mean history length, and with an RMSE against a 64 spp render of the final pose that is no worse."""
    sc = gg.opaque_scene()
    w, h = 96, 64
    base = [np.asarray(m, np.float64) for m, _ in sc.nodes]
    moving, static = gg.open_renderer(sc, (w, h), accel=accel), gg.open_renderer(sc, (w, h), accel=accel)
    try:
        cam = ghost.camera_for(sc, w, h, 0.0)
        vi, pi = np.array(cam.viewInverse, np.float32), np.array(cam.projInverse, np.float32)
        p = moving.temporal_params(moving.world_to_clip(sc.camera, w / h), 0.05, 0.05, 16.0)
        st = ghost.guide_state(w, h, 0)
        st.maxDepth, st.fireflyClampThreshold = 4, 4.0 * moving.env_integral
        hist = {id(moving): None, id(static): None}
        words = None
        for k in range(3):
            worlds = base[:3] + [translate(0.18 * k, 0.0, 0.0) @ base[3]]
            cur_words = words_of(worlds)
            for r in (moving, static):
                r.update_instances(node_array(sc, worlds))
                r.render_instance_plane(7, 50.0)
                st.frame = 0
                r.setPushContants(st)
                r.run()
                frame, ids = r.read_accum(), r.read_instance_plane()
                _, g1, g2 = r.read_guides(6)
                got = r.temporal_accumulate_moving(p) if r is moving else r.temporal_accumulate(p)
                hc, hn = r.read_temporal_history()
                tab = None if words is None else mh.table(words, cur_words)
                if r is static and tab is not None:
                    tab = np.zeros_like(tab)
                rc, new = mh.temporal_moving(frame, g1, g2, vi, pi, p, ids, tab, hist[id(r)])
                assert rc == 0
                assert np.array_equal(bits(got), bits(new.colour)) and np.array_equal(bits(hc), bits(new.colour)) and np.array_equal(bits(hn), bits(new.length)), (k, r is moving)
                hist[id(r)] = new
            words = cur_words
        box = ids == 3
        assert box.sum() > 200
        st.maxSamples = 64
        moving.setPushContants(st)
        moving.run()
        target = moving.read_accum()
    finally:
        moving.destroy()
        static.destroy()
    hm, hs = hist[id(moving)], hist[id(static)]
    sel = box & gen.finite3(hm.colour) & gen.finite3(hs.colour) & gen.finite3(target)
    n_moving, n_static = float(hm.length[sel].mean()), float(hs.length[sel].mean())
    e_moving, e_static = rmse(hm.colour, target, sel), rmse(hs.colour, target, sel)
    print(f"{int(sel.sum())} pixels of the moved box: mean history length moving {n_moving:.3f}, static {n_static:.3f}; RMSE against 64 spp moving {e_moving:.5f}, static {e_static:.5f}")
    assert n_moving > n_static
    assert e_moving <= e_static


# ---- the state machine ----------------------------------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing_and_leave_the_history_alone():
    L = capi.lib()
    size = (45, 37)
    w, h = size
    inp = mk.case_inputs(size, "slide")
    good = model.tmodel.params_of(inp)
    out = np.zeros((h, w, 4), np.float32)
    sc = three_node_scene()
    r = HipRenderer()
    r.setup(0)
    try:
        def call(p):
            return L.pt_temporal_accumulate_moving(r._ctx, None if p is None else C.byref(p), out.ctypes.data)
        assert L.pt_temporal_accumulate_moving(None, C.byref(good), out.ctypes.data) == capi.PT_ERR_INVALID
        # everything pt_temporal_accumulate refuses, in its order
        assert call(good) == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        r.create(size)
        r.write_accum(inp["colour"])
        assert call(good) == capi.PT_ERR_STATE and b"pt_set_camera" in L.pt_last_error(r._ctx)
        r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
        assert call(good) == capi.PT_ERR_STATE and b"guide planes" in L.pt_last_error(r._ctx)
        r.set_denoise_guides(None, inp["g1"], inp["g2"])
        assert call(None) == capi.PT_ERR_INVALID
        # ... then its own: no instance plane, no scene
        assert call(good) == capi.PT_ERR_STATE and b"instance plane" in L.pt_last_error(r._ctx)
        r.set_instance_plane(inp["ids"])
        assert call(good) == capi.PT_ERR_STATE and b"pt_set_scene" in L.pt_last_error(r._ctx)
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE       # none of that made a history
        # a history made without a scene has no instances: after pt_set_scene the moving form refuses it until pt_temporal_reset
        assert L.pt_temporal_accumulate(r._ctx, C.byref(good), None) == capi.PT_OK
        r.set_scene(sc)
        before = r.read_temporal_history()
        assert call(good) == capi.PT_ERR_STATE and b"pt_temporal_reset" in L.pt_last_error(r._ctx)
        bad = th.params(np.array(good.worldToClip, np.float32), 0.0, gen.NORMAL_DIST2, gen.MAX_HISTORY)
        assert call(bad) == capi.PT_ERR_INVALID
        r.set_instance_plane(None)
        assert call(good) == capi.PT_ERR_STATE and b"instance plane" in L.pt_last_error(r._ctx)
        after = r.read_temporal_history()
        assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
        r.set_instance_plane(inp["ids"])
        # the static form continues that history (it reads no table), and the history it leaves carries the scene's instances: the moving form continues it
        assert L.pt_temporal_accumulate(r._ctx, C.byref(good), None) == capi.PT_OK
        assert call(good) == capi.PT_OK
        # pt_temporal_reset: a first call, which only stores the image and the transforms
        r.temporal_reset()
        got = r.temporal_accumulate_moving(good)
        _, hn = r.read_temporal_history()
        assert np.array_equal(bits(got), bits(inp["colour"])) and np.array_equal(hn, np.where(gen.finite3(inp["colour"]), 1.0, 0.0).astype(np.float32))
        # a pt_resize to another size drops the plane with the history
        r.create((64, 48))
        small = mk.case_inputs((64, 48), "slide")
        r.write_accum(small["colour"])
        r.set_denoise_guides(None, small["g1"], small["g2"])
        assert L.pt_temporal_accumulate_moving(r._ctx, C.byref(model.tmodel.params_of(small)), None) == capi.PT_ERR_STATE and b"instance plane" in L.pt_last_error(r._ctx)
    finally:
        r.destroy()

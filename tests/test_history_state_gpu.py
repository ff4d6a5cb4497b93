"""The state a context keeps about its history (vk_raytrace_amd/csrc/pt_history.h), through the C ABI alone, on a 33 x 9 image -- one pixel past the
32 x 8 tile in both directions, the smallest shape with a partial tile on each axis -- with the moving form, so that the instance words kept with a
history are in play as well.  Everything that drops the history -- pt_temporal_reset, each of the three settings switched off, each switched on from
off, pt_resize to another size and back to the same one -- leaves all four readers refusing with the one "there is no history" text of
include/pt_api.h's PT_ERR_STATE, and the next call is a first call: equal to the host build run without a history (tests/history_host.py), bit for
bit, under the settings then in force.  A setting set to the value it has, new fast parameters while that setting stays on, and a pt_resize to the
size the image has (which include/pt_api.h and pt_resize define as no resize) keep the history: readable, and every byte as it was."""
import ctypes as C

import numpy as np
import pytest

from tests import albedo_host as ah, fast_host as fh, motion_host as mh
from tests import test_fast_model as model
from tests.test_motion_gpu import identity_worlds, node_array, three_node_scene
from tests.test_temporal_gpu import camera_words
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
ak, sk, bits = model.ak, model.sk, model.bits
SIZE = (33, 9)
SETTINGS = ("moments", "demodulate", "fast")
NO_HISTORY = "%s: there is no history (no pt_temporal_accumulate since pt_resize / pt_temporal_reset)"
FP = fh.params(2.5, 1.0, 2)
IDS = (np.arange(SIZE[0] * SIZE[1], dtype=np.uint32).reshape(SIZE[1], SIZE[0]) * 7) % 5    # nodes 0 .. 2, and 3 and 4: no instance
IDS[IDS == 4] = mh.NONE


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    sc = three_node_scene()
    r.set_scene(sc)
    r.update_instances(node_array(sc, identity_worlds()))
    yield r
    r.destroy()


def apply(r, on):
    """the three settings as `on` names them"""
    r.track_moments(on["moments"])
    r.temporal_demodulate(on["demodulate"])
    r.temporal_fast(FP if on["fast"] else None)


def accumulate(r, k):
    """call k of the sequence through pt_temporal_accumulate_moving, planes installed first (pt_resize frees them); returns (inputs, returned image)"""
    inp = ak.call_inputs(SIZE, "yaw", k)
    r.write_accum(inp["colour"])
    r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
    r.set_instance_plane(IDS)
    r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
    return inp, r.temporal_accumulate_moving(model.params_of(inp))


def first_call_on_the_host(inp, on):
    """the host build's call without a history under the settings `on`"""
    args = (inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], model.params_of(inp))
    if on["fast"]:
        rc, want = fh.step(inp["colour"], inp["g0"] if on["demodulate"] else None, *args, FP, None, moments=on["moments"], ids=IDS)
    elif on["demodulate"]:
        rc, want = ah.temporal(inp["colour"], inp["g0"], *args, None, moments=on["moments"], ids=IDS)
    else:
        rc, want = mh.temporal_moving(inp["colour"], *args, IDS, None, None, moments=on["moments"])
    assert rc == 0
    return want


def readers(r):
    """the four entries that read the history, as (name, call) returning the status"""
    L, w, h = capi.lib(), *SIZE
    img, length, mom = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 2), np.float32)
    dp = hd.DenoiseParams(iterations=1, sigmaColor=1.0, sigmaGuide=(1.0, 1.0, 1.0), flags=0)
    return [("pt_read_temporal_history", lambda: L.pt_read_temporal_history(r._ctx, img.ctypes.data, length.ctypes.data)),
            ("pt_read_temporal_fast", lambda: L.pt_read_temporal_fast(r._ctx, img.ctypes.data, length.ctypes.data)),
            ("pt_read_temporal_moments", lambda: L.pt_read_temporal_moments(r._ctx, mom.ctypes.data)),
            ("pt_denoise_history", lambda: L.pt_denoise_history(r._ctx, C.byref(dp), img.ctypes.data))]


def held(r, on):
    """every image of the history the settings `on` keep, as words"""
    out = [*r.read_temporal_history()]
    if on["fast"]:
        out += r.read_temporal_fast()
    if on["moments"]:
        out.append(r.read_temporal_moments())
    return [bits(a).copy() for a in out]


DROPPERS = ["reset", "resize"] + [f"{s}_off" for s in SETTINGS] + [f"{s}_on" for s in SETTINGS]


@pytest.mark.parametrize("dropper", DROPPERS)
def test_a_dropped_history_is_refused_by_every_reader_and_the_next_call_is_a_first_call(dev, dropper):
    r = dev
    on = {s: dropper != f"{s}_on" for s in SETTINGS}        # all three on; "<s>_on" starts with s off
    r.create(SIZE)
    apply(r, on)
    r.temporal_reset()
    for k in (0, 1):
        accumulate(r, k)
    assert len(held(r, on)) == 2 + 2 * on["fast"] + on["moments"]        # there is a history, made with these settings
    if dropper == "reset":
        r.temporal_reset()
    elif dropper == "resize":
        r.create((SIZE[0] + 1, SIZE[1]))      # away and back to the same size: a pt_resize that changes nothing is no resize (the other test)
        r.create(SIZE)
    else:
        on[dropper.rsplit("_", 1)[0]] = dropper.endswith("_on")
        apply(r, on)      # (the two settings that keep their value keep the history: the other test)
    for name, call in readers(r):
        assert call() == capi.PT_ERR_STATE, name
        assert capi.lib().pt_last_error(r._ctx).decode() == NO_HISTORY % name
    inp, got = accumulate(r, sk.STATIC_CALLS)
    want = first_call_on_the_host(inp, on)
    pairs = list(zip(held(r, on), [want.colour, want.length] + ([want.fast, want.fast_length] if on["fast"] else []) + ([want.moments] if on["moments"] else [])))
    for a, b in [(bits(got), want.colour)] + pairs:
        assert np.array_equal(a, bits(b)), f"{dropper}: the call after it differs from the host build's first call"


@pytest.mark.parametrize("value", [True, False], ids=["on", "off"])
def test_a_setting_set_to_the_value_it_has_keeps_the_history(dev, value):
    r = dev
    on = {s: value for s in SETTINGS}
    r.create(SIZE)
    apply(r, on)
    r.temporal_reset()
    for k in (0, 1):
        accumulate(r, k)
    before = held(r, on)
    steps = [lambda: r.track_moments(value), lambda: r.temporal_demodulate(value), lambda: r.temporal_fast(FP if value else None),
             lambda: r.create(SIZE)]      # (include/pt_api.h: only a pt_resize to another size leaves no history)
    if value:
        steps.append(lambda: r.temporal_fast(fh.params(3.0, 2.0, 3)))      # new parameters while the setting stays on
    for step in steps:
        step()
        after = held(r, on)
        assert len(after) == len(before) and all(np.array_equal(a, b) for a, b in zip(before, after))

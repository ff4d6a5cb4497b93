"""The packet stage's child order on the device (csrc/pt_packet.h packet_visit_table, csrc/pt_order.h; PT_TUNE packetOrder): the order in which a
packet enters the children of a node is a matter of speed only.  The fixture of tests/handover_scene.py -- a few hundred triangles, alpha cards
in front of and behind an opaque wall, so that hand-over, count pass and exact loop all occur -- at 64 x 64 pixels (64 packets of 8 x 8; the
optical axis meets the image inside a block, so the sign-incoherent packets on the two lines through it are there) seen along each of the eight
direction-sign octants and along an axis, depth 2, 2 frames through the staged kernels (tail=0), flat and two-level, and once more after pt_update_instances has
moved the nodes: with the table (packetOrder=1) the accumulation image equals the one of the sorted visit (packetOrder=0) bit for bit, and both
equal the oracle's.  (The two-level walk keeps the sorted visit whatever the knob says; its cases hold the knob to that.)"""
import os

import numpy as np
import pytest

from tests.handover_scene import handover_scene
from vk_raytrace_amd import capi, synth
from vk_raytrace_amd.scene import Camera, translate, rotate_y, rotate_z

pytestmark = pytest.mark.gpu

FRAMES, DEPTH, SIZE = 2, 2, 64
CNT_STRIDE, CNT_IN, CNT_REDO = 16, 0, 6   # csrc/pt_internal.h
OCTANTS = [(sx, sy, sz) for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)] + [None]
ACCELS = [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL]


def scene_seen_from(octant):
    """the fixture with the eye on the octant's diagonal, looking at a point a little off the origin: most packets travel against the octant's
    signs on all three axes, and the field of view is wide enough (half angle 45 degrees, the coordinate planes lie 35 degrees off the diagonal)
    for packets that straddle a sign change.  None: the fixture's own camera, along -z, whose sign-incoherent packets lie on the two image lines
    through the optical axis and whose four image quadrants are four octants"""
    sc = handover_scene()
    if octant is not None:
        sc.camera = Camera(eye=tuple(1.9 * s for s in octant), center=(0.11, 0.07, 0.23), up=(0, 1, 0), fov=90.0)
    return sc


@pytest.fixture(scope="module")
def env():
    return synth.procedural_sky(64, 32)


def with_tune(tune, fn):
    keep = os.environ.get("PT_TUNE")
    os.environ["PT_TUNE"] = tune   # read by pt_create
    try:
        return fn()
    finally:
        if keep is None:
            del os.environ["PT_TUNE"]
        else:
            os.environ["PT_TUNE"] = keep


def render(cfg, order, accel):
    """image and the bounce-0 counter block of the newest launch sequence"""
    from tests.common import render_hip
    img, r = with_tune(f"tail=0,packetOrder={order}", lambda: render_hip(cfg, FRAMES, accel=accel, return_obj=True))
    try:
        counts = np.zeros((DEPTH, CNT_STRIDE), np.uint32)
        assert capi.lib().pt_debug_bounce_counts(r._ctx, counts.ctypes.data, DEPTH) == DEPTH
    finally:
        r.destroy()
    return img, counts


@pytest.mark.parametrize("octant", OCTANTS, ids=["axis" if o is None else "".join("+" if s > 0 else "-" for s in o) for o in OCTANTS])
def test_child_order_changes_no_image(env, octant):
    from tests.common import Config, render_oracle
    from tests.test_gpu_parity import assert_identical
    cfg = Config(scene_seen_from(octant), env, SIZE, SIZE, depth=DEPTH)
    want = render_oracle(cfg, FRAMES)
    assert np.isfinite(want).all() and float(want[..., :3].std()) > 0.0
    for accel in ACCELS:
        sorted_img, c0 = render(cfg, 0, accel)
        table_img, c1 = render(cfg, 1, accel)
        what = f"octant {octant}, accel {accel}"
        assert np.array_equal(table_img.view(np.uint32), sorted_img.view(np.uint32)), what
        assert_identical(table_img, want, what + ", packetOrder=1")
        assert_identical(sorted_img, want, what + ", packetOrder=0")
        for c in (c0, c1):   # packets were traversed, and the packets through the optical axis (and rays that need the count pass) went on
            assert 0 < c[0, CNT_REDO] < c[0, CNT_IN], (what, c[0])
        print(f"{what}: bounce 0 of {c1[0, CNT_IN]} rays: not settled by the packet stage {c0[0, CNT_REDO]} (sorted) / {c1[0, CNT_REDO]} (table)")


@pytest.mark.parametrize("accel", ACCELS, ids=["flat", "two-level"])
def test_child_order_after_update_instances(env, accel):
    """the tables of the structure pt_update_instances leaves (flat: rebuilt; two-level: a new instance hierarchy over the kept BLASes)"""
    from tests.common import Config, render_oracle
    from tests.test_gpu_parity import assert_identical
    from vk_raytrace_amd.renderer import HipRenderer
    sc = scene_seen_from(None)
    cfg = Config(sc, env, SIZE, SIZE, depth=DEPTH)
    rng = np.random.default_rng(5)
    moved = [(translate(*(rng.normal(0, 0.2, 3))) @ m @ rotate_z(rng.uniform(-0.5, 0.5)) @ rotate_y(rng.uniform(-0.3, 0.3)), p) if i else (m, p) for i, (m, p) in enumerate(sc.nodes)]
    images = []
    for order in (0, 1):
        def run():
            r = HipRenderer(); r.setup(0); r.set_accel_mode(accel); r.set_scene(cfg.scene)
            integral, _ = r.set_env(cfg.env); r.set_camera(cfg.camera); r.set_sunsky(cfg.sunsky); r.create((cfg.width, cfg.height))
            try:
                original = list(sc.nodes)
                sc.nodes[:] = moved
                r.update_instances(sc)
                st = cfg.state(integral)
                for f in range(FRAMES):
                    st.frame = f
                    r.setPushContants(st)
                    r.run()
                return r.read_accum()
            finally:
                sc.nodes[:] = original
                r.destroy()
        images.append(with_tune(f"tail=0,packetOrder={order}", run))
    assert np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))
    original = list(sc.nodes)
    sc.nodes[:] = moved   # (the oracle reads the scene's nodes when it is given the scene)
    try:
        assert_identical(images[1], render_oracle(cfg, FRAMES), "after pt_update_instances, packetOrder=1")
    finally:
        sc.nodes[:] = original

"""The hand-over of the packet stage's pass A on the device (csrc/pt_render.hip k_closest_k -> k_closest_r; PT_TUNE handover): the fixture of
tests/handover_scene.py at 64 x 64 pixels -- 64 blocks of 8 x 8, so whole packets, and the image contains the optical axis, so packets whose
lanes disagree on a direction sign run too --, depth 2, 4 frames as one batch, through the staged kernels (tail=0: by default an image this small
runs in k_tail, which has no packet stage).  With and without the hand-over, with a packet stage on bounce 0 and on both bounces, flat and
two-level: every image equals the oracle bit for bit, every ray counter equals the oracle's, and the per-bounce counter block
of the newest launch sequence (pt_debug_bounce_counts) shows that rays were handed over exactly where the knob says so."""
import os

import numpy as np
import pytest

from tests.handover_scene import handover_scene
from vk_raytrace_amd import capi, synth

pytestmark = pytest.mark.gpu

FRAMES, DEPTH = 4, 2
CNT_STRIDE, CNT_IN, CNT_X_CLOSEST, CNT_REDO, CNT_HANDOVER = 16, 0, 2, 6, 9   # csrc/pt_internal.h
RAY_KEYS = ("samples", "closestRays", "shadowRays", "shadedHits", "misses", "alphaTests", "neeLookups")
# regen=0: bounce 0 traces the rays k_generate wrote -- the form of the hand-over that adds to a ray already in the path state, which a later bounce's packet
# stage (packetClosest=2) reaches only where a scrambled queue happens to yield a sign-coherent packet
TUNES = ["tail=0,handover=1", "tail=0,handover=0", "tail=0,handover=1,regen=0", "tail=0,handover=1,packetClosest=2", "tail=0,handover=0,packetClosest=2"]


@pytest.fixture(scope="module")
def cfg():
    from tests.common import Config
    return Config(handover_scene(), synth.procedural_sky(64, 32), 64, 64, depth=DEPTH)


@pytest.fixture(scope="module")
def oracle(cfg):
    from tests.common import render_oracle
    img, o = render_oracle(cfg, FRAMES, return_obj=True)
    stats = o.stats()
    o.close()
    img.setflags(write=False)
    return img, stats


def render(cfg, tune, accel):
    """image, ray counters and the counter block of the batch's launch sequence under PT_TUNE = tune (read by pt_create)"""
    from tests.common import render_hip
    keep = os.environ.get("PT_TUNE")
    os.environ["PT_TUNE"] = tune
    try:
        img, r = render_hip(cfg, FRAMES, accel=accel, return_obj=True)
    finally:
        if keep is None:
            del os.environ["PT_TUNE"]
        else:
            os.environ["PT_TUNE"] = keep
    try:
        stats = r.stats()
        counts = np.zeros((DEPTH, CNT_STRIDE), np.uint32)
        n = capi.lib().pt_debug_bounce_counts(r._ctx, counts.ctypes.data, DEPTH)
        assert n == DEPTH, f"the staged kernels ran {n} bounces"
    finally:
        r.destroy()
    return img, stats, counts


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
def test_handover_changes_routes_not_results(cfg, oracle, accel):
    from tests.test_gpu_parity import assert_identical
    want, want_stats = oracle
    first = None
    for tune in TUNES:
        img, stats, counts = render(cfg, tune, accel)
        assert_identical(img, want, f"PT_TUNE={tune}")
        first = img if first is None else first
        assert np.array_equal(img.view(np.uint32), first.view(np.uint32)), tune
        for k in RAY_KEYS:
            assert stats[k] == want_stats[k], (tune, k, stats[k], want_stats[k])
        paths = int(counts[0, CNT_IN])   # the batch is cut into pieces over the frame slots: the newest sequence traced some of its frames
        assert paths % (cfg.width * cfg.height) == 0 and 0 < paths <= cfg.width * cfg.height * FRAMES
        print(f"{tune}: bounce 0 of {paths} rays: redo {counts[0, CNT_REDO]}, handed over {counts[0, CNT_HANDOVER]}, exact {counts[0, CNT_X_CLOSEST]}; "
              f"bounce 1 of {counts[1, CNT_IN]}: redo {counts[1, CNT_REDO]}, handed over {counts[1, CNT_HANDOVER]}, exact {counts[1, CNT_X_CLOSEST]}")
        assert 0 < counts[0, CNT_REDO] < paths, "packets were traversed, and some rays went on to the trace machine"
        if "handover=1" in tune:
            assert 0 < counts[0, CNT_HANDOVER] < counts[0, CNT_REDO], "rays were handed over, and the packets around the optical axis were redone whole"
            assert counts[0, CNT_X_CLOSEST] > 0, "the fixture has fractional candidates: rays went straight to the exact loop"
        else:
            assert (counts[:, CNT_HANDOVER] == 0).all()
        if "packetClosest=2" in tune:
            assert counts[1, CNT_REDO] > 0, "bounce 1 ran the packet stage"
        else:
            assert counts[1, CNT_REDO] == 0 and counts[1, CNT_HANDOVER] == 0
    assert want_stats["alphaTests"] > 0

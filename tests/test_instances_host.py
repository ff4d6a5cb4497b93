"""The instance pass on the CPU: instance_pixel<TWO> of vk_raytrace_amd/csrc/pt_guides.h (what pt_render_instance_plane runs per lane; DESIGN.md
section 5.5) compiled for the host by tests/cpp/motion_host.cpp and held, pixel by pixel, to the oracle.

Claim under test: for every pixel the instance plane holds the node the oracle's closest-hit trace reports for the very ray the guide planes are made from
-- the frame-0 camera ray with its depth-of-field draws, walked with the seed those draws leave behind -- which is what pt_RayHit::instanceID means, and
0xffffffff where that trace misses; and the guide planes written alongside are guide_pixel's, bit for bit, whatever the mask (0 included).  On the flat
structure -- which the harness builds without per-slot shading lines, so the node index comes from the TriRec; tests/test_instances_gpu.py holds the
device's shading-line form to this build -- and on the two-level one, at both sizes and both apertures of tests/test_guides_host.py, on its alpha scenes."""
import numpy as np
import pytest

from tests import guides_host, motion_host as mh
from tests import test_guides_host as host

SIZES, APERTURES, MISS_DEPTH, bits = host.SIZES, host.APERTURES, host.MISS_DEPTH, host.bits


@pytest.mark.parametrize("name", host.ALPHA_SCENES)
def test_the_plane_is_the_oracles_closest_hit_node_and_the_guides_are_guide_pixels(name):
    c = host.case(name)
    nodes = len(c.scene.nodes)
    for (w, h) in SIZES:
        for ap in APERTURES:
            c.set_camera(w, h, ap)
            org, dirs, s_cam, _ = guides_host.rays(c.traced, w, h)
            _, node, _, _, _ = c.oracle.trace_closest(org, dirs, s_cam)
            want = np.where(node >= 0, node, mh.NONE).astype(np.uint32).reshape(h, w)
            assert 0.10 <= (node >= 0).mean() <= 0.90 and len(np.unique(node[node >= 0])) > 1
            for two in (0, 1):
                planes = guides_host.guides(c.traced, two, w, h, 7, MISS_DEPTH)
                ids, got = mh.instances(c.traced, two, w, h, 7, MISS_DEPTH)
                label = f"{name} {w}x{h} aperture {ap} two={two}"
                same = ids == want
                assert same.all(), f"{label}: the instance plane differs from the oracle's node at {np.count_nonzero(~same)} pixels, first (y, x) {np.argwhere(~same)[:4].tolist()}"
                assert (ids[ids != mh.NONE] < nodes).all()
                for j in range(3):
                    assert np.array_equal(bits(got[j]), bits(planes[j])), f"{label}: guide plane {j}"


def test_the_mask_selects_the_guide_planes_and_never_the_instance_plane():
    c = host.case("fuzz1")
    w, h = SIZES[1]
    c.set_camera(w, h, APERTURES[1])
    full_ids, full = mh.instances(c.traced, 1, w, h, 7, MISS_DEPTH)
    for mask in (0, 1, 2, 4, 5):
        ids, got = mh.instances(c.traced, 1, w, h, mask, MISS_DEPTH)
        assert np.array_equal(ids, full_ids), mask
        for j in range(3):
            assert (got[j] is None) == (not mask & (1 << j)) and (got[j] is None or np.array_equal(bits(got[j]), bits(full[j]))), (mask, j)

"""The chained guide pass through the header-only C++ shim (include/pt_renderer.hpp renderGuidesChain / readGuideChain, tests/cpp/chain_shim_test.cpp): it
compiles against the C ABI, links with libptmi.so, and either runs one round whose checksums equal those of the same round through the Python route (GPU
box) or fails loudly with PT_ERR_NO_DEVICE."""
import numpy as np
import pytest

from tests import shim
from tests.shim import fnv


def test_cpp_shim_with_the_chained_guide_pass_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "chain_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


def python_route():
    """the round of chain_shim_test.cpp through HipRenderer: the same two quads, materials, camera and chain parameters"""
    from vk_raytrace_amd import capi
    from vk_raytrace_amd.renderer import HipRenderer
    from vk_raytrace_amd.scene import Camera, Scene
    w, h = 24, 16
    sc = Scene("chain_shim")
    mats = [sc.add_material(pbrBaseColorFactor=(0.9, 0.8, 0.7, 1.0), pbrMetallicFactor=1.0, pbrRoughnessFactor=0.0),
            sc.add_material(pbrBaseColorFactor=(0.2, 0.4, 0.6, 1.0), pbrMetallicFactor=0.0, pbrRoughnessFactor=1.0)]
    pos, nrm, uv = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], [(0, 0, 1)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)]
    pms = [sc.add_prim_mesh(pos, nrm, uv, [0, 1, 2, 0, 2, 3], m, tangents=[(1, 0, 0, 1)] * 4) for m in mats]
    sc.add_node(pms[0])
    far = np.diag([-4.0, 4.0, -4.0, 1.0])
    far[2, 3] = 5.0
    sc.add_node(pms[1], far)
    sc.finalize(capi.pack_vertices)
    cam = Camera(eye=(0, 0, 3), center=(0, 0, 0), up=(0, 1, 0), fov=60.0)
    out = {}
    r = HipRenderer()
    r.setup(0)
    try:
        r.set_scene(sc)
        r.create((w, h))
        r.set_camera(capi.camera_lookat(cam, float(np.float32(w) / np.float32(h))))
        for mode, tag in ((capi.PT_ACCEL_FLAT, ""), (capi.PT_ACCEL_TWO_LEVEL, "2")):
            r.set_accel_mode(mode)
            r.capture_guides_chain(r.guide_chain(4, 0.05, 0.9, 0.9), 7, 50.0)
            planes, links = r.read_guides(), r.read_guide_chain()
            assert links[h // 2, w // 2] == 1 and links[0, 0] == 1 << 8
            out.update({"albedo" + tag: fnv(planes[0]), "normal" + tag: fnv(planes[1]), "depth" + tag: fnv(planes[2]), "links" + tag: fnv(links)})
        return out
    finally:
        r.destroy()


@pytest.mark.gpu
def test_cpp_shim_round_equals_the_python_route(tmp_path):
    verdict, got = shim.run(shim.build_shim(tmp_path, "chain_shim_test"))
    assert verdict == "OK"
    assert got == python_route()

"""The header-only C++ Renderer shim (include/pt_renderer.hpp) compiles against the C ABI, links with
libptmi.so, and either renders (GPU box) or fails loudly with PT_ERR_NO_DEVICE (no CPU fallback)."""
import pytest

from tests import shim


def test_cpp_shim_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "renderer_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


@pytest.mark.gpu
def test_cpp_shim_renders_on_gpu(tmp_path):
    from vk_raytrace_amd import gltf, synth
    glb = str(tmp_path / "quad.glb")
    gltf.save_gltf(synth.quad_scene(), glb)     # the same quad through Scene::load's replacement (pt_gltf_load via HipPathTracer::loadGltf)
    verdict, _ = shim.run(shim.build_shim(tmp_path, "renderer_shim_test"), glb)
    assert verdict == "OK"

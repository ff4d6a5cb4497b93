"""The guide pass through the header-only C++ shim (include/pt_renderer.hpp renderGuides / readDenoiseGuides, tests/cpp/guides_shim_test.cpp): it
compiles against the C ABI, links with libptmi.so, and either renders the planes of a quad (GPU box) or fails loudly with PT_ERR_NO_DEVICE."""
import pytest

from tests import shim


def test_cpp_shim_with_the_guide_pass_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "guides_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


@pytest.mark.gpu
def test_cpp_shim_renders_and_reads_guides_on_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "guides_shim_test"))
    assert verdict == "OK"

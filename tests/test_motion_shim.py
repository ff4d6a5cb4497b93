"""Motion of moving instances through the header-only C++ shim (include/pt_renderer.hpp renderInstancePlane / setInstancePlane / readInstancePlane /
temporalAccumulateMoving, tests/cpp/motion_shim_test.cpp): it compiles against the C ABI, links with libptmi.so, and either runs its round -- a quad that
slides within its own plane keeps its history in the moving form and loses part of it in the static one (GPU box) -- or fails loudly with PT_ERR_NO_DEVICE."""
import pytest

from tests import shim


def test_cpp_shim_with_the_motion_entry_points_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "motion_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


@pytest.mark.gpu
def test_cpp_shim_keeps_the_history_of_a_sliding_quad_on_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "motion_shim_test"))
    assert verdict == "OK"

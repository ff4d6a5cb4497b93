"""The guide pass through the header-only C++ shim (include/pt_renderer.hpp renderGuides / readDenoiseGuides, tests/cpp/guides_shim_test.cpp): it
compiles against the C ABI, links with libptmi.so, and either renders the planes of a quad (GPU box) or fails loudly with PT_ERR_NO_DEVICE."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_guides_shim(tmp_path):
    exe = str(tmp_path / "guides_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "guides_shim_test.cpp"),
                           "-L", os.path.join(ROOT, "vk_raytrace_amd"), "-l:libptmi.so", "-Wl,-rpath," + os.path.join(ROOT, "vk_raytrace_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    return exe


def test_cpp_shim_with_the_guide_pass_builds_and_fails_loudly_without_gpu(tmp_path):
    out = subprocess.run([build_guides_shim(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("NO_DEVICE") or out.stdout.startswith("OK")


@pytest.mark.gpu
def test_cpp_shim_renders_and_reads_guides_on_gpu(tmp_path):
    out = subprocess.run([build_guides_shim(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr

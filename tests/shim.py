"""The rig of the C++ shim tests (tests/test_*shim*.py, tests/test_query_host.py): the one link line of the programs under tests/cpp/*_shim_test.cpp,
how they are run and read, and the Python side of what tests/cpp/stage/shim_common.h holds -- the checksum and the planes and images of a round, word
for word.  A plain module: no test lives here."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_shim(tmp_path, name, extra_flags=()):
    """tests/cpp/<name>.cpp against include/pt_renderer.hpp, linked with libptmi.so: the program's path"""
    exe = str(tmp_path / name)
    lib_dir = os.path.join(ROOT, "vk_raytrace_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", *extra_flags, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-L", lib_dir, "-l:libptmi.so", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    return exe


def run(exe, *args):
    """the program's verdict -- the first word it prints, OK or NO_DEVICE -- and the key=value pairs after it; any other end is an error"""
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    words = out.stdout.split()
    assert out.returncode == 0 and words and words[0] in ("OK", "NO_DEVICE"), out.stdout + out.stderr
    return words[0], dict(kv.split("=", 1) for kv in words[1:] if "=" in kv)


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def planes(w, h):
    """shim_planes: (normal, depth), (H, W, 4) float32 each"""
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 4), np.float32)
    normal[...] = (0.5, 0.5, 1.0, 1.0)
    depth = np.zeros((h, w, 4), np.float32)
    depth[..., 0] = np.float32(4.0) + ((xs * 3 + ys * 5) % 16).astype(np.float32) * np.float32(0.125)
    return normal, depth


def image(w, h, k):
    """shim_image: (H, W, 4) float32"""
    i = np.arange(w * h * 4, dtype=np.uint64)
    return (((i * np.uint64(37 + 4 * k)) % np.uint64(101)).astype(np.float32) / np.float32(50.0)).reshape(h, w, 4)

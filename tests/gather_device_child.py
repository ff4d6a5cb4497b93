"""Child process of tests/test_gather_gpu.py::test_device_pointers_from_a_torch_tensor_and_the_timing_entry: pt_gather with PT_RAYS_DEVICE, and
pt_debug_gather_time, on memory a torch tensor owns, for both kinds.

torch is imported FIRST, on purpose, for the reason tests/query_device_child.py gives: the tensor's memory and the context must live in ONE HIP runtime."""
import ctypes as C
import os
import sys

import torch  # noqa: E402  (before vk_raytrace_amd: see above)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from vk_raytrace_amd import capi, host_device as hd, synth  # noqa: E402
from vk_raytrace_amd.renderer import HipRenderer  # noqa: E402


def main():
    scene = synth.fuzz_scene(0)
    scene.finalize(capi.pack_vertices)
    env = synth.procedural_sky(128, 64)
    rng = np.random.default_rng(99)
    n = 4097
    pts = np.zeros(n, hd.gatherpoint_dtype)
    pts["position"] = (rng.normal(0, 1, (n, 3)) * 2.0).astype(np.float32)
    pts["normal"] = rng.normal(0, 1, (n, 3)).astype(np.float32)
    pts["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    pts["normal"][7] = 0   # an invalid point for the hemisphere kind
    for accel in (capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(scene)
        integral, _ = r.set_env(env)
        r.set_camera(capi.camera_lookat(scene.camera, 4 / 3, nb_lights=len(scene.lights)))
        st = hd.default_rtx_state()
        st.maxDepth, st.maxSamples, st.fireflyClampThreshold = 5, 3, 4.0 * integral
        for kind, size in ((capi.PT_GATHER_HEMISPHERE, 32), (capi.PT_GATHER_SPHERE, 128)):
            want = r.gather_records(st, kind, pts)
            assert (want["hitFraction"] > 0).any() and (want["hitFraction"] < 1).any() and (want["status"] != 0).sum() == (1 if kind == capi.PT_GATHER_HEMISPHERE else 0)
            t_pts = torch.frombuffer(bytearray(pts.tobytes()), dtype=torch.uint8).cuda()
            t_out = torch.full((n * size,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert t_pts.data_ptr() % 16 == 0 and t_out.data_ptr() % 16 == 0
            r.gather_device(st, kind, t_pts.data_ptr(), t_out.data_ptr(), n)
            got = t_out.cpu().numpy().tobytes()
            assert got == want.tobytes(), f"accel {accel} kind {kind}: device-pointer records differ from the host-pointer call"
            assert t_pts.cpu().numpy().tobytes() == pts.tobytes(), "the points are read only"
            for po, oo in ((4, 0), (0, 4)):   # a pointer offset by 4 bytes is refused, nothing is launched (the records stay as they are)
                try:
                    r.gather_device(st, kind, t_pts.data_ptr() + po, t_out.data_ptr() + oo, n - 1)
                    raise AssertionError("misaligned device pointer accepted")
                except capi.PtError as e:
                    assert e.code == capi.PT_ERR_INVALID, e
            assert t_out.cpu().numpy().tobytes() == got
            # the timing entry: the same launch three times between two events
            t_out.fill_(0xAB)
            torch.cuda.synchronize()
            ms = C.c_float(-1.0)
            r._check(capi.lib().pt_debug_gather_time(r._ctx, C.byref(st), kind, n, C.c_void_p(t_pts.data_ptr()), C.c_void_p(t_out.data_ptr()), 3, C.byref(ms)))
            assert ms.value > 0.0, ms.value
            assert t_out.cpu().numpy().tobytes() == got, "pt_debug_gather_time runs pt_gather's launch"
        r.destroy()
    print("OK")


if __name__ == "__main__":
    main()

"""Child process of tests/test_paths_gpu.py::test_device_pointers_from_a_torch_tensor_and_the_timing_entry: pt_trace_paths with PT_RAYS_DEVICE, and
pt_debug_paths_time, on memory a torch tensor owns.

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
    rays = np.zeros(n, hd.ray_dtype)
    rays["origin"] = (np.array([0, 0, 6]) + rng.normal(0, 1, (n, 3)) * 3.0).astype(np.float32)
    d = rng.normal(0, 1, (n, 3)) * 1.5 - rays["origin"]
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["tmax"] = np.inf
    rays["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for accel in (capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(scene)
        integral, _ = r.set_env(env)
        r.set_camera(capi.camera_lookat(scene.camera, 4 / 3, nb_lights=len(scene.lights)))
        st = hd.default_rtx_state()
        st.maxDepth, st.maxSamples, st.fireflyClampThreshold = 5, 2, 4.0 * integral
        want = r.trace_path_records(st, rays)
        assert (want["status"] == capi.PT_RAY_HIT).sum() > n // 4 and (want["radiance"] > 0).any()
        t_rays = torch.frombuffer(bytearray(rays.tobytes()), dtype=torch.uint8).cuda()
        t_out = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert t_rays.data_ptr() % 16 == 0 and t_out.data_ptr() % 16 == 0
        r.trace_paths_device(st, t_rays.data_ptr(), t_out.data_ptr(), n)
        got = t_out.cpu().numpy().tobytes()
        assert got == want.tobytes(), f"accel {accel}: device-pointer records differ from the host-pointer call"
        assert t_rays.cpu().numpy().tobytes() == rays.tobytes(), "the rays are read only"
        for ro, oo in ((4, 0), (0, 4)):   # a pointer offset by 4 bytes is refused, nothing is launched (the records stay as they are)
            try:
                r.trace_paths_device(st, t_rays.data_ptr() + ro, t_out.data_ptr() + oo, n - 1)
                raise AssertionError("misaligned device pointer accepted")
            except capi.PtError as e:
                assert e.code == capi.PT_ERR_INVALID, e
        assert t_out.cpu().numpy().tobytes() == got
        # the timing entry: the same launch three times between two events
        t_out.fill_(0xAB)
        torch.cuda.synchronize()
        ms = C.c_float(-1.0)
        r._check(capi.lib().pt_debug_paths_time(r._ctx, C.byref(st), n, C.c_void_p(t_rays.data_ptr()), C.c_void_p(t_out.data_ptr()), 3, C.byref(ms)))
        assert ms.value > 0.0, ms.value
        assert t_out.cpu().numpy().tobytes() == got, "pt_debug_paths_time runs pt_trace_paths' launch"
        r.destroy()
    print("OK")


if __name__ == "__main__":
    main()

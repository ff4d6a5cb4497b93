"""Child process of tests/test_query_gpu.py::test_device_pointers_from_a_torch_tensor: pt_trace_rays with PT_RAYS_DEVICE on memory a torch tensor owns.

torch is imported FIRST, on purpose: the PyTorch-ROCm wheel bundles its own HIP runtime, and two initialised HIP runtimes do not coexist in one process
(vk_raytrace_amd/capi.py lib()).  With torch's runtime already loaded, libptmi.so's dependency on the HIP runtime resolves to that copy, so the tensor's
memory and the context live in ONE runtime -- which is what a caller who keeps rays in torch tensors has to do as well.  The pytest process itself has
libptmi bound to the system runtime, hence the fresh process."""
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
    rng = np.random.default_rng(99)
    n = 4097
    rays = np.zeros(n, hd.ray_dtype)
    rays["origin"] = (np.array([0, 0, 6]) + rng.normal(0, 1, (n, 3)) * 3.0).astype(np.float32)
    d = rng.normal(0, 1, (n, 3)) * 1.5 - rays["origin"]
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["tmax"] = rng.uniform(2.0, 12.0, n).astype(np.float32)
    rays["seed"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for accel in (capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(scene)
        hits_seen = 0
        for kind, hpr in ((capi.PT_RAYS_CLOSEST, 1), (capi.PT_RAYS_OCCLUDED, 1), (capi.PT_RAYS_NEAREST, 1), (capi.PT_RAYS_CANDIDATES, 5)):
            want = r.trace_ray_records(kind, rays, hpr)
            hits_seen += int((want["status"] & capi.PT_RAY_HIT).sum())
            t_rays = torch.frombuffer(bytearray(rays.tobytes()), dtype=torch.uint8).cuda()
            t_hits = torch.full((n * hpr * 32,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert t_rays.data_ptr() % 16 == 0 and t_hits.data_ptr() % 16 == 0
            r.trace_rays_device(kind, t_rays.data_ptr(), t_hits.data_ptr(), n, hpr)
            got = t_hits.cpu().numpy().tobytes()
            assert got == want.tobytes(), f"accel {accel} kind {kind}: device-pointer results differ from the host-pointer call"
            assert t_rays.cpu().numpy().tobytes() == rays.tobytes(), "the rays are read only"
            for ro, ho in ((4, 0), (0, 4)):   # a pointer offset by 4 bytes is refused, nothing is launched (the results stay as they are)
                try:
                    r.trace_rays_device(kind, t_rays.data_ptr() + ro, t_hits.data_ptr() + ho, n - 1, hpr)
                    raise AssertionError("misaligned device pointer accepted")
                except capi.PtError as e:
                    assert e.code == capi.PT_ERR_INVALID, e
            assert t_hits.cpu().numpy().tobytes() == got
        assert hits_seen > n, hits_seen
        r.destroy()
    print("OK")


if __name__ == "__main__":
    main()

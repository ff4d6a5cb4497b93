"""bench.py's plain run on the GPU: the headline line alone, one timed window of exactly --steps frames, and --dump-outputs writing the accumulation
image the timed path left after its last step -- the same bits from run to run with the same arguments, and the frames the CPU oracle renders."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orc
from vk_raytrace_amd import capi, host_device as hd, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, WARMUP, STEPS, TEX, TRIS = 256, 160, 1, 3, 32, 2000


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--width", str(W), "--height", str(H),
           "--tex-size", str(TEX), "--tris", str(TRIS), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])


def _oracle_image(frames):
    """the bench workload of _plain_run rendered by the CPU oracle: frames 0 .. frames-1 accumulated like the GPU's framebuffer"""
    wl = workloads.c3_sponza(W, H, STEPS, tex_size=TEX, target_tris=TRIS)
    wl.scene.finalize(capi.pack_vertices)
    o = orc.Oracle()
    o.set_scene(wl.scene)
    integral, _ = o.set_env(wl.env)
    o.set_camera(capi.camera_lookat(wl.scene.camera, W / H, nb_lights=len(wl.scene.lights)))
    o.set_sunsky(hd.default_sun_and_sky())
    st = hd.default_rtx_state()
    st.size[0], st.size[1] = W, H
    st.maxDepth, st.pbrMode, st.maxSamples = wl.depth, wl.pbr_mode, 1
    st.fireflyClampThreshold = 4.0 * integral
    return o.render(st, frames)


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_same_image_every_time(tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and len(line["repeats"]) == 1 and line["value"] > 0
        assert abs(line["ms_per_step"] - W * H / (line["value"] * 1e6) * 1e3) < 1e-9 * line["ms_per_step"]
        for k in ("calibration", "cpu_baseline", "parity", "serialised", "roofline", "interactive"):
            assert k not in line, k
    assert sorted(os.listdir(tmp_path / "a")) == ["image.npy"]
    img_a, img_b = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "b" / "image.npy")
    assert img_a.dtype == np.float32 and img_a.shape == (H, W, 4)
    assert np.array_equal(img_a.view(np.uint32), img_b.view(np.uint32))
    mean = float(np.mean(img_a[..., :3]))
    assert mean == a["image_mean"] or (np.isnan(mean) and np.isnan(a["image_mean"]))  # the line's image_mean is taken on the same image
    ref = _oracle_image(WARMUP + STEPS)
    same = (img_a.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(img_a) & np.isnan(ref))
    assert same.all(), f"{int((~same).any(axis=-1).sum())} of {W * H} pixels differ from the oracle"

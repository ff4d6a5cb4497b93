"""pt_trace_paths on the device, through the C ABI, for the flat and the two-level structure: against the frames of the same
context -- one sample on frame 0's camera rays is pt_read_accum after frame 0, the same tree, so there is no allowance -- and against the host build of
the same source (tests/paths_host.py: pt_paths.h's path_query compiled by g++), every field of every record, bit for bit.

Against the host build the TREE may differ (the device's builder against its host emulation), and a tree only matters to a ray with an ill-conditioned
candidate (tests/test_query_gpu.py): a record that differs is accepted only with that proof, along the first ray of its path whose candidate lists
differ, and only a few of them.  pt_trace_rays recorded 0 differences on these fixtures; 0 is what is expected here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import paths_host
from tests.common import Config
from tests.host_harness import NONE, alpha_scenes, deep_rays, ill_conditioned, instanced_scene, rays_for
from tests.test_paths_host import HIT, config, one_triangle_config, sky
from tests.test_query_host import CANDIDATES, DEGENERATE_DIR, DEGENERATE_ORG, INF, alpha_inputs, bits, host_query, make_rays, records_equal, world_index
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCELS = [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL]
ACCEL_IDS = ["flat", "two-level"]
DIFFER_CAP = 3   # records of 6000 per structure that may differ from the host build, each with its proof


def two_of(accel):
    return 1 if accel == capi.PT_ACCEL_TWO_LEVEL else 0


def renderer(cfg, accel, variant=None):
    """everything pt_trace_paths needs of the scene side; no pt_resize"""
    r = HipRenderer()
    r.setup(0)
    r.set_accel_mode(accel)
    r.set_variant(cfg.variant if variant is None else variant)
    r.set_scene(cfg.scene)
    r.useAnyHit(cfg.any_hit)
    integral, _ = r.set_env(cfg.env)
    r.set_camera(cfg.camera)
    r.set_sunsky(cfg.sunsky)
    return r, integral


def proven_differences(r, ps, two, st, variant, rays, dev, host, what):
    """Records that differ from the host build's.  Each must come with the proof: along the first ray of the path (ph_path_segments) whose candidate
    lists differ between the two trees, fp32's verdict on one of the two triangles at the first differing position is an artefact (ill_conditioned)."""
    bad = np.nonzero((dev.view(np.uint32).reshape(len(rays), -1) != host.view(np.uint32).reshape(len(rays), -1)).any(1))[0]
    for i in bad[:DIFFER_CAP + 1]:
        for seg in ps.segments(two, st, rays[i], variant=variant):
            one = np.array([seg], hd.ray_dtype)
            one["tmax"], one["seed"] = INF, 0
            dc, hc = r.trace_ray_records(CANDIDATES, one, 16)[0], host_query(ps.tr, two, CANDIDATES, one, hits_per_ray=16)[0]
            dw, hw = world_index(ps.cfg.scene, dc), world_index(ps.cfg.scene, hc)
            diff = np.nonzero((dw != hw) | (bits(dc["t"]) != bits(hc["t"])))[0]
            if len(diff):
                c = int(diff[0])
                o, d = one["origin"][0], one["direction"][0]
                assert any(x != NONE and ill_conditioned(ps.tr.world_tri(x), o, d, tx) for x, tx in ((dw[c], dc["t"][c]), (hw[c], hc["t"][c]))), \
                    f"{what}: ray {i}: a well-conditioned candidate differs at position {c}: device {dw} {dc['t']} vs host {hw} {hc['t']}"
                break
        else:
            raise AssertionError(f"{what}: ray {i} differs ({dev[i]} vs {host[i]}) although both trees report the same candidates along its path")
    return len(bad)


def check_against_host(r, ps, accel, rays, what, depth=5, samples=(1, 3), variants=(capi.PT_VARIANT_RAYQUERY, capi.PT_VARIANT_RTX)):
    two, seen = two_of(accel), {}
    for variant in variants:
        r.set_variant(variant)
        for s in samples:
            st = ps.state(maxDepth=depth, maxSamples=s)
            dev, host = r.trace_path_records(st, rays), ps.paths(two, st, rays, variant=variant)
            n = proven_differences(r, ps, two, st, variant, rays, dev, host, f"{what} variant {variant} samples {s}")
            seen[(variant, s)] = n
            assert n <= DIFFER_CAP, (what, variant, s, n)
            assert (dev["status"] == HIT).mean() > 0.2 and (dev["seed"] != rays["seed"]).mean() > 0.2 and (dev["_pad"] == 0).all()
    print(f"{what}: records differing from the host build (all through ill-conditioned candidates): {seen}")
    assert sum(seen.values()) <= DIFFER_CAP, seen   # per structure


# ---- device equals device: the frames of the same context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name", ["feature box disney", "feature box gltf", "fuzz 2 rtx sun & sky", "fuzz 4 depth of field"])
def test_one_sample_on_the_camera_rays_is_the_contexts_frame(name, accel):
    cfg = config(name)
    ps = paths_host.PathScene(cfg)
    r, integral = renderer(cfg, accel)
    st = cfg.state(integral)
    rays = ps.camera_rays(st)
    got = r.trace_path_records(st, rays)            # before any pt_resize
    r.create((cfg.width, cfg.height))
    r.setPushContants(st); r.run()
    frame = r.read_accum()
    assert np.array_equal(bits(got["radiance"].reshape(cfg.height, cfg.width, 3)), bits(frame[..., :3])), f"{np.count_nonzero((bits(got['radiance'].reshape(cfg.height, cfg.width, 3)) != bits(frame[..., :3])).any(-1))} pixels differ"
    assert frame[..., :3].max() > 0 and 0.1 < (got["status"] == HIT).mean()
    assert records_equal(r.trace_path_records(st, rays), got)   # ... and after
    r.destroy(); ps.close()


# ---- device equals host build -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,scene,eye,spread", list(alpha_scenes()), ids=lambda x: x if isinstance(x, str) else None)
def test_device_equals_host_on_the_alpha_scenes(name, scene, eye, spread, accel):
    cfg = Config(scene, sky(), 64, 48)
    ps = paths_host.PathScene(cfg)
    r, _ = renderer(cfg, accel)
    org, dirs, seeds, _ = alpha_inputs(ps.tr, eye, spread)
    check_against_host(r, ps, accel, make_rays(org, dirs, seeds=seeds), f"{name} {ACCEL_IDS[two_of(accel)]}")
    r.destroy(); ps.close()


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_device_equals_host_on_the_instanced_scene(accel):
    sc, _, off = instanced_scene(0)
    cfg = Config(sc, sky(), 64, 48)
    ps = paths_host.PathScene(cfg)
    r, _ = renderer(cfg, accel)
    org, dirs = rays_for(ps.tr, np.random.default_rng(100), off, 6000)
    check_against_host(r, ps, accel, make_rays(org, dirs, seeds=np.arange(len(org), dtype=np.uint32)), f"instanced scene 0 {ACCEL_IDS[two_of(accel)]}")
    r.destroy(); ps.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_wave_edges_and_the_refill(accel):
    cfg = Config(synth.fuzz_scene(0), sky(), 64, 48)
    ps = paths_host.PathScene(cfg)
    r, _ = renderer(cfg, accel)
    two = two_of(accel)
    org, dirs, seeds, _ = alpha_inputs(ps.tr, (0, 0, 6), 3.0, n=4097)
    rays = make_rays(org, dirs, seeds=seeds)
    st = ps.state(maxDepth=5, maxSamples=2)
    host = ps.paths(two, st, rays)
    full = None
    for n in (1, 63, 64, 65, 4097):
        dev = r.trace_path_records(st, rays[:n])
        assert len(dev) == n and proven_differences(r, ps, two, st, cfg.variant, rays[:n], dev, host[:n], f"n={n}") <= DIFFER_CAP
        full = dev
    # one wavefront for 300 rays: every lane comes back for more; the records are the default launch's
    assert r._lib.pt_debug_paths_waves(r._ctx, 1) == capi.PT_OK
    one_wave = r.trace_path_records(st, rays[:300])
    assert r._lib.pt_debug_paths_waves(r._ctx, 0) == capi.PT_OK
    assert records_equal(one_wave, full[:300]) and records_equal(r.trace_path_records(st, rays[:300]), full[:300])
    r.destroy(); ps.close()


def test_host_arrays_cross_the_staging_chunk():
    """n = 2^20 + 65 on the one-triangle scene at depth 2: two pieces through the staging buffers.  Equal to the same rays sent as two smaller calls, and
    4096 rays on both sides of the boundary equal the host build."""
    cfg = one_triangle_config()
    ps = paths_host.PathScene(cfg)
    r, _ = renderer(cfg, capi.PT_ACCEL_FLAT)
    n = capi.PT_QUERY_CHUNK + 65
    rng = np.random.default_rng(5)
    org = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), np.full((n, 1), 3.0)], 1).astype(np.float32)
    rays = make_rays(org, np.tile(np.array([0, 0, -1], np.float32), (n, 1)), seeds=np.arange(n, dtype=np.uint32))
    st = ps.state(maxDepth=2)
    big = r.trace_path_records(st, rays)
    assert 0.1 < (big["status"] == HIT).mean() < 0.4 and (big["closestRays"] >= 1).all() and (big["radiance"] > 0).any(1).mean() > 0.9
    k = 600001
    assert records_equal(big, np.concatenate([r.trace_path_records(st, rays[:k]), r.trace_path_records(st, rays[k:])]))
    lo, hi = capi.PT_QUERY_CHUNK - 2048, capi.PT_QUERY_CHUNK + 2048
    assert records_equal(big[lo:hi], ps.paths(0, st, rays[lo:hi]))
    r.destroy(); ps.close()


def test_device_pointers_from_a_torch_tensor_and_the_timing_entry():
    """rays in a torch tensor on the GPU, records in another: byte for byte the host-pointer call's, both structures; a pointer offset by 4 bytes is
    refused; pt_debug_paths_time on the same tensors returns a positive time and leaves the same records.  A process of its own:
    tests/query_device_child.py says why."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "paths_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("display", [False, True], ids=["plain", "display-images-pending"])
def test_a_path_query_disturbs_nothing(display):
    cfg = Config(synth.fuzz_scene(0), sky(), 64, 48, depth=5)
    tm = hd.default_tonemapper()
    rng = np.random.default_rng(1)
    o = (np.array([0, 0, 6]) + rng.normal(0, 1, (4097, 3))).astype(np.float32)
    rays = make_rays(o, -o / np.linalg.norm(o, axis=1, keepdims=True), seeds=rng.integers(0, 2 ** 32, 4097, dtype=np.uint64).astype(np.uint32))

    def run(query):
        r, integral = renderer(cfg, capi.PT_ACCEL_FLAT)
        r.create((cfg.width, cfg.height))
        st = cfg.state(integral)
        images = []
        for f in range(4):
            if f == 2 and query:
                before = r.stats()
                if display:
                    r.tonemap_begin(tm)
                qs = cfg.state(integral); qs.maxSamples = 2
                got = r.trace_path_records(qs, rays)
                assert (got["status"] == HIT).mean() > 0.3 and (got["seed"] != rays["seed"]).any() and (got["radiance"] > 0).any()
                assert r.tonemap_pending() == (2 if display else 0)
                assert r.stats() == before, "pt_Stats across the path query"
            elif f == 2 and display:
                r.tonemap_begin(tm)
            st.frame = f
            r.setPushContants(st); r.run()
            if display and f == 0:
                r.tonemap_begin(tm)
        while r.tonemap_pending():
            images.append(r.tonemap_end())
        acc = r.read_accum()
        r.destroy()
        return acc, images

    acc, images = run(True)
    ref, ref_images = run(False)
    assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32)) and len(images) == len(ref_images) == (2 if display else 0)
    assert all(np.array_equal(a, b) for a, b in zip(images, ref_images))


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_the_spill_scene_equals_the_host_build(accel):
    """camera rays of the spill scene reach the private spill array on their first walk"""
    cfg = Config(synth.deep_chain(synth.DEEP_SPILL_LEVELS), synth.procedural_sky(64, 32), 64, 48)
    o, d = deep_rays(cfg)
    rays = make_rays(o, d, seeds=np.arange(len(o), dtype=np.uint32))
    ps = paths_host.PathScene(cfg)
    r, _ = renderer(cfg, accel)
    st = ps.state(maxDepth=4, maxSamples=2)
    dev = r.trace_path_records(st, rays)   # PT_OK: no overflow
    assert (dev["status"] == HIT).mean() > 0.5
    assert proven_differences(r, ps, two_of(accel), st, cfg.variant, rays, dev, ps.paths(two_of(accel), st, rays), "spill scene") <= DIFFER_CAP
    r.destroy(); ps.close()


# ---- refusals and timing --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = capi.lib()
    cfg = one_triangle_config()
    rays = make_rays(DEGENERATE_ORG, DEGENERATE_DIR)
    out = np.zeros(3, hd.pathresult_dtype)
    out["status"] = 0xABABABAB
    untouched = out.copy()
    rp, op = rays.ctypes.data, out.ctypes.data
    assert rp % 16 == 0 and op % 16 == 0   # (the alignment is checked before anything is launched: host addresses serve as misaligned "device" pointers)
    good = hd.default_rtx_state()
    good.maxDepth = 3
    r = HipRenderer(); r.setup(0)
    ctx = r._ctx

    def call(st=good, flags=0, n=3, rays_p=rp, out_p=op):
        return L.pt_trace_paths(ctx, C.byref(st) if st is not None else None, flags, n, rays_p, out_p)

    def refused(code, text, **kw):
        assert call(**kw) == code, (text, kw)
        said = L.pt_last_error(ctx)
        assert said.startswith(b"pt_trace_paths") and text in said, (text, said)

    assert L.pt_trace_paths(None, C.byref(good), 0, 3, rp, op) == capi.PT_ERR_INVALID
    # the state of the context, piece by piece
    refused(capi.PT_ERR_STATE, b"pt_set_scene")
    d, keep = cfg.scene.desc()
    assert L.pt_set_scene(ctx, C.byref(d)) == capi.PT_OK
    refused(capi.PT_ERR_STATE, b"pt_build_accel")
    assert L.pt_build_accel(ctx) == capi.PT_OK
    refused(capi.PT_ERR_STATE, b"environment")
    r.set_env(cfg.env)
    refused(capi.PT_ERR_STATE, b"pt_set_camera")
    cam = hd.SceneCamera.from_buffer_copy(cfg.camera); cam.nbLights = 2
    r.set_camera(cam)
    refused(capi.PT_ERR_INVALID, b"nbLights")
    r.set_camera(cfg.camera)
    # the arguments
    def state(**fields):
        st = hd.RtxState.from_buffer_copy(good)
        for k, v in fields.items():
            setattr(st, k, v)
        return st

    refused(capi.PT_ERR_INVALID, b"null state", st=None)
    refused(capi.PT_ERR_INVALID, b"flag", flags=2)
    refused(capi.PT_ERR_INVALID, b"flag", flags=0x80000001)
    refused(capi.PT_ERR_INVALID, b": null", rays_p=None)
    refused(capi.PT_ERR_INVALID, b": null", out_p=None)
    refused(capi.PT_ERR_INVALID, b"aligned", flags=capi.PT_RAYS_DEVICE, rays_p=rp + 4)
    refused(capi.PT_ERR_INVALID, b"aligned", flags=capi.PT_RAYS_DEVICE, out_p=op + 8)
    refused(capi.PT_ERR_INVALID, b"n = ", n=(1 << 40) + 1)
    refused(capi.PT_ERR_INVALID, b"maxDepth", st=state(maxDepth=-1))
    refused(capi.PT_ERR_INVALID, b"maxDepth", st=state(maxDepth=1000))
    refused(capi.PT_ERR_INVALID, b"maxSamples", st=state(maxSamples=0))
    refused(capi.PT_ERR_INVALID, b"maxSamples", st=state(maxSamples=capi.PT_PATHS_MAX_SAMPLES + 1))
    refused(capi.PT_ERR_INVALID, b"pbrMode", st=state(pbrMode=2))
    refused(capi.PT_ERR_INVALID, b"PT_DEBUG_HEATMAP", st=state(debugging_mode=hd.eHeatmap))
    assert records_equal(out, untouched), "a refused call writes nothing"
    assert call(n=0, rays_p=None, out_p=None) == capi.PT_OK                          # n == 0: nothing to do
    assert call(n=0, rays_p=None, out_p=None, flags=capi.PT_RAYS_DEVICE) == capi.PT_OK
    assert records_equal(out, untouched)
    # frame, size and the heat-map bounds are ignored; no pt_resize needed
    assert call(st=state(frame=-7, size=(0, -1), minHeatmap=9, maxHeatmap=3, maxSamples=capi.PT_PATHS_MAX_SAMPLES, maxDepth=1)) == capi.PT_OK
    assert np.array_equal(out["status"], [HIT, HIT, 0]) and np.array_equal(out["closestRays"], [capi.PT_PATHS_MAX_SAMPLES] * 3)
    r.destroy()


def test_the_timing_entry_refuses_what_the_call_refuses():
    """pt_debug_paths_time checks its own arguments, then the call's; the positive time on device arrays is the torch child's
    (test_device_pointers_from_a_torch_tensor_and_the_timing_entry)"""
    cfg = one_triangle_config()
    r, integral = renderer(cfg, capi.PT_ACCEL_FLAT)
    st, ms = cfg.state(integral), C.c_float(-1.0)
    L, ctx = r._lib, r._ctx
    for args, text in (((C.byref(st), 64, 16, 32, 0, C.byref(ms)), b"reps"), ((C.byref(st), 0, 16, 32, 1, C.byref(ms)), b"reps"), ((C.byref(st), 64, 16, 32, 1, None), b"null"),
                       ((C.byref(st), 64, 20, 32, 1, C.byref(ms)), b"aligned"), ((None, 64, 16, 32, 1, C.byref(ms)), b"null state")):
        assert L.pt_debug_paths_time(ctx, *args) == capi.PT_ERR_INVALID, args
        assert L.pt_last_error(ctx).startswith(b"pt_debug_paths_time") and text in L.pt_last_error(ctx), L.pt_last_error(ctx)
    assert ms.value == -1.0
    r.destroy()

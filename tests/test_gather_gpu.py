"""pt_gather on the device, through the C ABI, for both kinds, the flat and the two-level structure and both shadow variants:
every field of every record against the host build of the same source (tests/gather_host.py: pt_gather.h's gather_point compiled by g++), bit for bit,
and against the device's own path queries (the composition of section 3.3 out of pt_trace_paths, through the C ABI).

Against the host build the TREE may differ (the device's builder against its host emulation), and a tree only matters to a ray with an ill-conditioned
candidate (tests/test_paths_gpu.py): a record that differs is accepted only with that proof along the first segment of its first differing sample, and
at most one of 600 per structure.  Path queries recorded 0 differences on these scenes; 0 is what is expected here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gather_host as gh
from tests import test_paths_gpu as tpg
from tests.common import Config
from tests.host_harness import alpha_scenes, instanced_scene
from tests.paths_host import advance
from tests.test_gather_host import HEMISPHERE, KIND_IDS, KINDS, PI32, SH_C, SPHERE, invalid_point_batch, one_sample_state, scene_config, scene_points
from tests.test_paths_host import INVALID, one_triangle_config, sky
from tests.test_query_host import bits, records_equal
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCELS, ACCEL_IDS, two_of, renderer = tpg.ACCELS, tpg.ACCEL_IDS, tpg.two_of, tpg.renderer
DIFFER_CAP = 1   # records of (at most) 600 per structure that may differ from the host build, each with its proof
VARIANTS = (capi.PT_VARIANT_RAYQUERY, capi.PT_VARIANT_RTX)


def proven_differences(r, gs, two, st, variant, kind, pts, dev, host, what):
    """Records that differ from the host build's.  Each must come with the proof: its samples' rays (gh_gather_rays), one sample at a time through
    pt_trace_paths on the device and ph_paths on the host, differ somewhere, and the first such ray has the CANDIDATES proof of
    tests/test_paths_gpu.py along the first segment that differs."""
    bad = np.nonzero((dev.view(np.uint32).reshape(len(pts), -1) != host.view(np.uint32).reshape(len(pts), -1)).any(1))[0]
    one = one_sample_state(st)
    for i in bad[:DIFFER_CAP + 1]:
        rays = gs.rays(two, st, kind, pts[i], variant=variant)
        d1, h1 = r.trace_path_records(one, rays), gs.paths(two, one, rays, variant=variant)
        first = np.nonzero((d1.view(np.uint32).reshape(len(rays), -1) != h1.view(np.uint32).reshape(len(rays), -1)).any(1))[0]
        assert len(first), f"{what}: point {i} differs ({dev[i]} vs {host[i]}) although every sample's path agrees with the host build"
        s = int(first[0])
        assert tpg.proven_differences(r, gs, two, one, variant, rays[s:s + 1], d1[s:s + 1], h1[s:s + 1], f"{what} point {i} sample {s}") == 1
    return len(bad)


def check_against_host(r, gs, accel, pts, what, depth=5, samples=(1, 3)):
    two, seen = two_of(accel), {}
    for variant in VARIANTS:
        r.set_variant(variant)
        for kind in KINDS:
            for s in samples:
                st = gs.state(maxDepth=depth, maxSamples=s)
                dev, host = r.gather_records(st, kind, pts), gs.gather(two, st, kind, pts, variant=variant)
                n = proven_differences(r, gs, two, st, variant, kind, pts, dev, host, f"{what} variant {variant} kind {kind} samples {s}")
                seen[(variant, kind, s)] = n
                assert n <= DIFFER_CAP, (what, variant, kind, s, n)
                assert (dev["hitFraction"] > 0).mean() > 0.2 and (dev["seed"] != pts["seed"]).all() and (dev["_pad"] == 0).all() and (dev["status"] == 0).all()
    print(f"{what}: records differing from the host build (all through ill-conditioned candidates): {sum(seen.values())} {seen}")
    assert sum(seen.values()) <= DIFFER_CAP, seen   # per structure


# ---- device equals host build -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name", ["feature box", "fuzz 2 rtx sun & sky"])
def test_device_equals_host_on_the_host_tests_points(name, accel):
    cfg = scene_config(name)
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, accel)
    check_against_host(r, gs, accel, scene_points(name), f"{name} {ACCEL_IDS[two_of(accel)]}")
    r.destroy(); gs.close()


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,scene,eye,spread", list(alpha_scenes()), ids=lambda x: x if isinstance(x, str) else None)
def test_device_equals_host_on_the_alpha_scenes(name, scene, eye, spread, accel):
    cfg = Config(scene, sky(), 64, 48)
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, accel)
    check_against_host(r, gs, accel, gh.scene_points(scene, np.random.default_rng(4242), on_surface=536, free=64), f"{name} {ACCEL_IDS[two_of(accel)]}")
    r.destroy(); gs.close()


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_device_equals_host_on_the_instanced_scene(accel):
    sc, _, _ = instanced_scene(0)
    cfg = Config(sc, sky(), 64, 48)
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, accel)
    check_against_host(r, gs, accel, gh.scene_points(sc, np.random.default_rng(100), on_surface=536, free=64), f"instanced scene 0 {ACCEL_IDS[two_of(accel)]}")
    r.destroy(); gs.close()


# ---- device equals device: the composition through the C ABI -----------------------------------------------------------------------------------------
def sh_basis32(d):
    """gather_sh_basis of pt_gather.h in numpy float32, operation for operation: (n, 9)"""
    x, y, z = (np.ascontiguousarray(d[:, i], np.float32) for i in range(3))
    one, three = np.float32(1.0), np.float32(3.0)
    return np.stack([np.full_like(x, SH_C[0]), SH_C[1] * y, SH_C[2] * z, SH_C[3] * x, SH_C[4] * (x * y), SH_C[5] * (y * z), SH_C[6] * (three * (z * z) - one), SH_C[7] * (x * z),
                     SH_C[8] * (x * x - y * y)], 1)


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_four_samples_are_four_device_path_queries(accel):
    """the host tests' composition, on the device alone: the rays the host build emits for each point, one sample at a time through pt_trace_paths,
    reduced in numpy float32 in section 3.3's order"""
    name, S = "feature box", 4
    cfg = scene_config(name)
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, accel)
    pts, two = scene_points(name), two_of(accel)
    st = gs.state(maxDepth=5, maxSamples=S, fireflyClampThreshold=np.float32(0.5))
    one = one_sample_state(st)
    for kind in KINDS:
        got = r.gather_records(st, kind, pts)
        rays = np.stack([gs.rays(two, st, kind, p) for p in pts])
        total = np.zeros((len(pts), 3), np.float32) if kind == HEMISPHERE else np.zeros((len(pts), 9, 3), np.float32)
        hits, closest = np.zeros(len(pts), np.float32), np.zeros(len(pts), np.uint32)
        for s in range(S):
            rec = r.trace_path_records(one, rays[:, s])
            if s + 1 < S:
                assert np.array_equal(advance(rec["seed"], 2), rays["seed"][:, s + 1])
            L = rec["radiance"]
            total = total + (L if kind == HEMISPHERE else L[:, None, :] * sh_basis32(rays["direction"][:, s])[:, :, None])
            hits, closest = hits + (rec["status"] & 1).astype(np.float32), closest + rec["closestRays"]
        want = (total / np.float32(S)) * (PI32 if kind == HEMISPHERE else np.float32(4.0) * PI32)
        field = "irradiance" if kind == HEMISPHERE else "sh"
        assert np.array_equal(bits(got[field]), bits(want)), f"kind {kind}: {np.count_nonzero((bits(got[field]) != bits(want)).reshape(len(pts), -1).any(1))} points differ"
        assert np.array_equal(got["seed"], rec["seed"]) and np.array_equal(got["closestRays"], closest) and np.array_equal(bits(got["hitFraction"]), bits(hits / np.float32(S)))
        assert (got[field] != 0).any(-1).mean() > 0.3
    r.destroy(); gs.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_wave_edges_and_the_refill(accel, kind):
    scene = synth.fuzz_scene(0)
    cfg = Config(scene, sky(), 64, 48)
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, accel)
    two = two_of(accel)
    pts = gh.scene_points(scene, np.random.default_rng(7), on_surface=3585, free=512)
    pts["normal"][5] = 0; pts["position"][70][1] = np.nan   # invalid points among the others (the first for HEMISPHERE only)
    st = gs.state(maxDepth=5, maxSamples=3)
    host = gs.gather(two, st, kind, pts)
    full = None
    for n in (1, 63, 64, 65, 4097):
        dev = r.gather_records(st, kind, pts[:n])
        assert len(dev) == n and proven_differences(r, gs, two, st, cfg.variant, kind, pts[:n], dev, host[:n], f"n={n}") <= DIFFER_CAP
        full = dev
    assert full["status"][70] == INVALID and full["status"][5] == (INVALID if kind == HEMISPHERE else 0) and (full["status"] != 0).sum() == (2 if kind == HEMISPHERE else 1)
    # one wavefront for 300 points: every lane comes back for more; the records are the default launch's
    assert r._lib.pt_debug_gather_waves(r._ctx, 1) == capi.PT_OK
    one_wave = r.gather_records(st, kind, pts[:300])
    assert r._lib.pt_debug_gather_waves(r._ctx, 0) == capi.PT_OK
    assert records_equal(one_wave, full[:300]) and records_equal(r.gather_records(st, kind, pts[:300]), full[:300])
    r.destroy(); gs.close()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_host_arrays_cross_the_staging_chunk(kind):
    """PT_QUERY_CHUNK + 65 HEMISPHERE points, PT_QUERY_CHUNK / 4 + 65 SPHERE points (32 MB of records a piece either way) above the one-triangle scene,
    one sample, depth 1: two pieces through the staging buffers.  Status 0 on all, and a seeded subset of 4096 records that includes both sides of the
    boundary equals the host build."""
    cfg = one_triangle_config()
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, capi.PT_ACCEL_FLAT)
    piece = capi.PT_QUERY_CHUNK if kind == HEMISPHERE else capi.PT_QUERY_CHUNK // 4
    n = piece + 65
    rng = np.random.default_rng(5)
    pos = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), np.full((n, 1), 3.0)], 1).astype(np.float32)
    pts = gh.make_points(pos, np.tile(np.array([0.1, 0.2, -1], np.float32), (n, 1)), np.arange(n, dtype=np.uint32))
    st = gs.state(maxDepth=1, maxSamples=1)
    big = r.gather_records(st, kind, pts)
    miss = big["hitFraction"] == 0   # (a miss draws nothing after the two direction draws; a hit goes on to draw for its light and its lobe)
    assert (big["status"] == 0).all() and (big["closestRays"] == 1).all() and np.array_equal(big["seed"][miss], advance(pts["seed"], 2)[miss]) and 0 < miss.mean() < 1
    near = np.arange(piece - 1024, piece + 65)   # both sides of the boundary
    pick = np.sort(np.concatenate([near, rng.choice(np.setdiff1d(np.arange(n), near), 4096 - len(near), replace=False)]))
    assert len(pick) == 4096 and len(np.unique(pick)) == 4096
    assert records_equal(big[pick], gs.gather(0, st, kind, pts[pick]))
    r.destroy(); gs.close()


def test_device_pointers_from_a_torch_tensor_and_the_timing_entry():
    """points in a torch tensor on the GPU, records in another: byte for byte the host-pointer call's, both kinds, both structures; a pointer offset by
    4 bytes is refused; pt_debug_gather_time on the same tensors returns a positive time and leaves the same records.  A process of its own:
    tests/query_device_child.py says why."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gather_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("display", [False, True], ids=["plain", "display-images-pending"])
def test_a_gather_disturbs_nothing(display):
    scene = synth.fuzz_scene(0)
    cfg = Config(scene, sky(), 64, 48, depth=5)
    tm = hd.default_tonemapper()
    pts = gh.scene_points(scene, np.random.default_rng(1), on_surface=1024, free=65)

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
                for kind in KINDS:
                    got = r.gather_records(qs, kind, pts)
                    assert (got["hitFraction"] > 0).mean() > 0.2 and (got["seed"] != pts["seed"]).all() and (got["irradiance" if kind == HEMISPHERE else "sh"] != 0).any()
                assert r.tonemap_pending() == (2 if display else 0)
                assert r.stats() == before, "pt_Stats across the gather"
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


def test_invalid_points_on_the_device():
    cfg = one_triangle_config()
    gs = gh.GatherScene(cfg)
    r, _ = renderer(cfg, capi.PT_ACCEL_FLAT)
    pts, bad = invalid_point_batch()
    st = gs.state(maxDepth=3, maxSamples=2)
    for kind in KINDS:
        dev = r.gather_records(st, kind, pts)
        assert records_equal(dev, gs.gather(0, st, kind, pts)) and np.array_equal(np.nonzero(dev["status"] == INVALID)[0], bad[kind])
    r.destroy(); gs.close()


# ---- refusals and timing --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = capi.lib()
    cfg = one_triangle_config()
    pts = gh.make_points([(0, 0, 3), (0.2, 0.1, 3), (5, 5, 5)], [(0, 0, -1)] * 3)
    out = np.zeros(3, hd.proberesult_dtype)
    out["status"] = 0xABABABAB
    untouched = out.copy()
    pp, op = pts.ctypes.data, out.ctypes.data
    assert pp % 16 == 0 and op % 16 == 0   # (the alignment is checked before anything is launched: host addresses serve as misaligned "device" pointers)
    good = hd.default_rtx_state()
    good.maxDepth = 3
    r = HipRenderer(); r.setup(0)
    ctx = r._ctx

    def call(st=good, kind=HEMISPHERE, flags=0, n=3, pts_p=pp, out_p=op):
        return L.pt_gather(ctx, C.byref(st) if st is not None else None, kind, flags, n, pts_p, out_p)

    def refused(code, text, **kw):
        assert call(**kw) == code, (text, kw)
        said = L.pt_last_error(ctx)
        assert said.startswith(b"pt_gather") and text in said, (text, said)

    assert L.pt_gather(None, C.byref(good), 0, 0, 3, pp, op) == capi.PT_ERR_INVALID
    refused(capi.PT_ERR_INVALID, b"unknown kind", kind=2)          # the kind comes first: it says what `results` is
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

    def state(**fields):
        st = hd.RtxState.from_buffer_copy(good)
        for k, v in fields.items():
            setattr(st, k, v)
        return st

    for kind in KINDS:
        refused(capi.PT_ERR_INVALID, b"null state", st=None, kind=kind)
        refused(capi.PT_ERR_INVALID, b"flag", flags=2, kind=kind)
        refused(capi.PT_ERR_INVALID, b": null", pts_p=None, kind=kind)
        refused(capi.PT_ERR_INVALID, b": null", out_p=None, kind=kind)
        refused(capi.PT_ERR_INVALID, b"aligned", flags=capi.PT_RAYS_DEVICE, pts_p=pp + 4, kind=kind)
        refused(capi.PT_ERR_INVALID, b"aligned", flags=capi.PT_RAYS_DEVICE, out_p=op + 8, kind=kind)
        refused(capi.PT_ERR_INVALID, b"n = ", n=(1 << 40) + 1, kind=kind)
        refused(capi.PT_ERR_INVALID, b"maxDepth", st=state(maxDepth=-1), kind=kind)
        refused(capi.PT_ERR_INVALID, b"maxDepth", st=state(maxDepth=1000), kind=kind)
        refused(capi.PT_ERR_INVALID, b"maxSamples", st=state(maxSamples=0), kind=kind)
        refused(capi.PT_ERR_INVALID, b"maxSamples", st=state(maxSamples=capi.PT_PATHS_MAX_SAMPLES + 1), kind=kind)
        refused(capi.PT_ERR_INVALID, b"pbrMode", st=state(pbrMode=2), kind=kind)
        refused(capi.PT_ERR_INVALID, b"PT_DEBUG_HEATMAP", st=state(debugging_mode=hd.eHeatmap), kind=kind)
    refused(capi.PT_ERR_INVALID, b"unknown kind", kind=0xFFFFFFFF)
    assert records_equal(out, untouched), "a refused call writes nothing"
    for kind in KINDS:
        assert call(n=0, pts_p=None, out_p=None, kind=kind) == capi.PT_OK                          # n == 0: nothing to do
        assert call(n=0, pts_p=None, out_p=None, kind=kind, flags=capi.PT_RAYS_DEVICE) == capi.PT_OK
    assert records_equal(out, untouched)
    # frame, size and the heat-map bounds are ignored; no pt_resize needed
    assert call(st=state(frame=-7, size=(0, -1), minHeatmap=9, maxHeatmap=3, maxSamples=4096, maxDepth=1), kind=SPHERE) == capi.PT_OK
    assert (out["status"] == 0).all() and np.array_equal(out["closestRays"], [4096] * 3) and (out["hitFraction"][:2] > 0).all()
    r.destroy()


def test_the_timing_entry_refuses_what_the_call_refuses():
    """pt_debug_gather_time checks its own arguments, then the call's; the positive time on device arrays is the torch child's"""
    cfg = one_triangle_config()
    r, integral = renderer(cfg, capi.PT_ACCEL_FLAT)
    st, ms = cfg.state(integral), C.c_float(-1.0)
    L, ctx = r._lib, r._ctx
    for args, text in (((C.byref(st), 0, 64, 16, 32, 0, C.byref(ms)), b"reps"), ((C.byref(st), 1, 0, 16, 32, 1, C.byref(ms)), b"reps"), ((C.byref(st), 0, 64, 16, 32, 1, None), b"null"),
                       ((C.byref(st), 1, 64, 20, 32, 1, C.byref(ms)), b"aligned"), ((None, 0, 64, 16, 32, 1, C.byref(ms)), b"null state"), ((C.byref(st), 7, 64, 16, 32, 1, C.byref(ms)), b"unknown kind")):
        assert L.pt_debug_gather_time(ctx, *args) == capi.PT_ERR_INVALID, args
        assert L.pt_last_error(ctx).startswith(b"pt_debug_gather_time") and text in L.pt_last_error(ctx), L.pt_last_error(ctx)
    assert ms.value == -1.0
    r.destroy()

"""pt_trace_rays on the device against the host build of the same source: the device leg of tests/test_query_host.py, through the C ABI, for the flat
and the two-level structure.

The reference is the host harness (tests/cpp/query_host.cpp: pt_query.h's query_ray compiled by g++, on structures assembled by the host emulation of the
device builder).  Device and host run the same functions on the same scene records, so every field of every pt_RayHit is expected to agree bit for bit.
What may differ is the TREE (the device's builder against its host emulation), and a tree only matters to a ray with an ill-conditioned candidate (an
accidental hit of fp32's Moeller-Trumbore, see tests/test_trace_host.py): such a ray is accepted only with that proof, per ray, and only a few of them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.common import Config
from tests.host_harness import NONE, TracedScene, alpha_scenes, deep_rays, ill_conditioned, instanced_scene, rays_for
from tests.test_query_host import (ALL_KINDS, CANDIDATES, CLOSEST, DEGENERATE_DIR, DEGENERATE_ORG, HIT, INF, INVALID, NEAREST, OCCLUDED, alpha_inputs, bits, empty_scenes,
                                   host_query, invalid_ray_batch, make_rays, one_triangle_scene, records_equal, three_layer_scene, world_index)
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCELS = [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL]
ACCEL_IDS = ["flat", "two-level"]
CANDIDATE_CAP = 12   # rays per structure that may differ through an ill-conditioned candidate on CANDIDATES / NEAREST (the cap of the host walks)
SETTLE_CAP = 3       # ... of 6000 on CLOSEST / OCCLUDED


def renderer(scene, accel, variant=capi.PT_VARIANT_RAYQUERY):
    if scene.vertices is None:
        scene.finalize(capi.pack_vertices)
    r = HipRenderer()
    r.setup(0)
    r.set_accel_mode(accel)
    r.set_variant(variant)
    r.set_scene(scene)
    return r


def two_of(accel):
    return 1 if accel == capi.PT_ACCEL_TWO_LEVEL else 0


def proven_differences(r, tr, scene, two, rays, dev, host, what):
    """Rays whose device records differ from the host's.  Each must come with the proof: the candidate lists of the two trees along that ray differ, and
    fp32's verdict on one of the two triangles at the first differing position is an artefact (ill_conditioned)."""
    k = dev.shape[1] if dev.ndim == 2 else 1
    bad = np.nonzero((np.ascontiguousarray(dev).view(np.uint32).reshape(len(rays), -1) != np.ascontiguousarray(host).view(np.uint32).reshape(len(rays), -1)).any(1))[0]
    for i in bad:
        one = rays[i:i + 1].copy()
        one["tmax"] = INF
        dc, hc = r.trace_ray_records(CANDIDATES, one, 16)[0], host_query(tr, two, CANDIDATES, one, hits_per_ray=16)[0]
        dw, hw = world_index(scene, dc), world_index(scene, hc)
        diff = np.nonzero((dw != hw) | (bits(dc["t"]) != bits(hc["t"])))[0]
        assert len(diff), f"{what}: ray {i} differs ({dev[i]} vs {host[i]}) although both trees report the same candidates"
        c = int(diff[0])
        o, d = one["origin"][0], one["direction"][0]
        assert any(x != NONE and ill_conditioned(tr.world_tri(x), o, d, tx) for x, tx in ((dw[c], dc["t"][c]), (hw[c], hc["t"][c]))), \
            f"{what}: ray {i}: a well-conditioned candidate differs at position {c}: device {dw} {dc['t']} vs host {hw} {hc['t']}"
    return len(bad)


def check_all_kinds(r, tr, scene, accel, org, dirs, seeds, tmax, what, variants=(capi.PT_VARIANT_RAYQUERY,)):
    two = two_of(accel)
    seen = {}
    for kind, hpr, tm in ((CLOSEST, 1, tmax), (NEAREST, 1, tmax), (CANDIDATES, 6, INF), (CANDIDATES, 2, tmax)):
        rays = make_rays(org, dirs, tmax=tm, seeds=seeds)
        dev, host = r.trace_ray_records(kind, rays, hpr), host_query(tr, two, kind, rays, hits_per_ray=hpr)
        n = proven_differences(r, tr, scene, two, rays, dev, host, f"{what} kind {kind}")
        seen[(kind, hpr)] = n
        assert n <= (SETTLE_CAP if kind == CLOSEST else CANDIDATE_CAP), (kind, n)
        assert ((dev.reshape(len(rays), -1)[:, 0]["status"] & HIT) != 0).mean() > 0.2
    for variant in variants:
        r.set_variant(variant)
        rays = make_rays(org, dirs, tmax=tmax, seeds=seeds)
        dev, host = r.trace_ray_records(OCCLUDED, rays), host_query(tr, two, OCCLUDED, rays, variant=variant)
        n = proven_differences(r, tr, scene, two, rays, dev, host, f"{what} OCCLUDED variant {variant}")
        seen[(OCCLUDED, variant)] = n
        assert n <= SETTLE_CAP, n
        if variant == capi.PT_VARIANT_RTX:
            assert np.array_equal(dev["seed"], rays["seed"])
    r.set_variant(capi.PT_VARIANT_RAYQUERY)
    print(f"{what}: rays differing from the host harness (all through ill-conditioned candidates): {seen}")


# ---- device against host, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,scene,eye,spread", list(alpha_scenes()), ids=lambda x: x if isinstance(x, str) else None)
def test_device_equals_host_on_the_alpha_scenes(name, scene, eye, spread, accel):
    """the inputs of test_closest_and_occluded_equal_the_key_ordered_loop: 6000 rays and seeds, every kind, both variants of the shadow ray"""
    tr = TracedScene(scene)
    r = renderer(scene, accel)
    org, dirs, seeds, tmax = alpha_inputs(tr, eye, spread)
    check_all_kinds(r, tr, scene, accel, org, dirs, seeds, tmax, f"{name} {ACCEL_IDS[two_of(accel)]}", variants=(capi.PT_VARIANT_RAYQUERY, capi.PT_VARIANT_RTX))
    # pt_use_any_hit(0): the structure is rebuilt all-opaque, nothing draws -- CLOSEST returns every seed as it came and equals CANDIDATES' first entry
    r.useAnyHit(False)
    rays = make_rays(org, dirs, tmax=tmax, seeds=seeds)
    c, o, k = r.trace_ray_records(CLOSEST, rays), r.trace_ray_records(OCCLUDED, rays), r.trace_ray_records(CANDIDATES, make_rays(org, dirs, seeds=seeds), 1)[:, 0]
    assert np.array_equal(c["seed"], seeds) and np.array_equal(o["seed"], seeds) and records_equal(c, k)
    r.destroy(); tr.close()


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("seed", [0, 3])
def test_device_equals_host_on_the_instanced_scenes(seed, accel):
    """scaled / rotated / mirrored / coincident instances, camera-like, surface-to-surface, axis-parallel and far-origin rays (rays_for)"""
    sc, _, off = instanced_scene(seed)
    tr = TracedScene(sc)   # the instance flags are the product's own here (from the materials), as on the device
    r = renderer(sc, accel)
    org, dirs = rays_for(tr, np.random.default_rng(100 + seed), off, 6000)
    tmax = np.where(np.arange(len(org)) % 3 == 0, INF, np.float32(9.0)).astype(np.float32)
    check_all_kinds(r, tr, sc, accel, org, dirs, np.arange(len(org), dtype=np.uint32), tmax, f"instanced scene {seed} {ACCEL_IDS[two_of(accel)]}")
    r.destroy(); tr.close()


@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_edges_on_the_device(accel):
    """degenerate scenes, the exclusive upper bound, empty ranges, one invalid ray per rule among valid neighbours, 16 results for 3 candidates"""
    two = two_of(accel)
    sc, _ = one_triangle_scene()
    tr, r = TracedScene(sc), renderer(sc, accel)
    t_hit = host_query(tr, two, NEAREST, make_rays(DEGENERATE_ORG[:1], DEGENERATE_DIR[:1]))["t"][0]
    assert t_hit > 0
    tm = np.array([t_hit, np.nextafter(t_hit, np.float32(np.inf)), 0.0, -1.0, -np.inf, np.inf], np.float32)
    bound = make_rays(np.repeat(DEGENERATE_ORG[:1], len(tm), 0), np.repeat(DEGENERATE_DIR[:1], len(tm), 0), tmax=tm, seeds=3)
    invalid, where = invalid_ray_batch()
    for kind in ALL_KINDS:
        hpr = 2 if kind == CANDIDATES else 1
        for rays in (make_rays(DEGENERATE_ORG, DEGENERATE_DIR, seeds=[5, 6, 7]), bound, invalid):
            dev = r.trace_ray_records(kind, rays, hpr)
            assert records_equal(dev, host_query(tr, two, kind, rays, hits_per_ray=hpr)), (kind, dev)
        dev = r.trace_ray_records(kind, bound, hpr).reshape(len(tm), -1)[:, 0]
        assert np.array_equal(dev["status"], [HIT] * 6 if kind == CLOSEST else [0, HIT, 0, 0, 0, HIT]), (kind, dev["status"])
        dev = r.trace_ray_records(kind, invalid, hpr).reshape(len(invalid), -1)
        bad = np.array([i for i, kinds in where if kind in kinds])
        assert (dev["status"][bad] == INVALID).all() and (dev["seed"][bad] == invalid["seed"][bad][:, None]).all() and (np.delete(dev["status"][:, 0], bad) & INVALID == 0).all()
    r.destroy(); tr.close()
    for sc, _ in empty_scenes():
        tr, r = TracedScene(sc), renderer(sc, accel)
        for kind in ALL_KINDS:
            dev = r.trace_ray_records(kind, invalid)
            assert records_equal(dev, host_query(tr, two, kind, invalid)) and ((dev["status"] & HIT) == 0).all()
        r.destroy(); tr.close()
    sc, _ = three_layer_scene()
    tr, r = TracedScene(sc), renderer(sc, accel)
    rays = make_rays([[0, -0.2, 5]], [[0, 0, -1]], seeds=9)   # (seen from +z the three layers face the ray, whatever the material's sidedness)
    dev = r.trace_ray_records(CANDIDATES, rays, 16)
    assert records_equal(dev, host_query(tr, two, CANDIDATES, rays, hits_per_ray=16))
    assert np.array_equal(dev[0]["status"], [HIT] * 3 + [0] * 13) and np.array_equal(dev[0]["instanceID"][:3], [0, 1, 2])
    r.destroy(); tr.close()


# ---- wave and chunk edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_wave_edges(accel):
    scene = synth.fuzz_scene(0)
    tr, r = TracedScene(scene), renderer(scene, accel)
    org, dirs, seeds, tmax = alpha_inputs(tr, (0, 0, 6), 3.0, n=4097)
    rays = make_rays(org, dirs, tmax=tmax, seeds=seeds)
    for kind, hpr in ((CLOSEST, 1), (OCCLUDED, 1), (CANDIDATES, 3)):
        host = host_query(tr, two_of(accel), kind, rays, hits_per_ray=hpr)
        for n in (1, 63, 64, 65, 4097):
            dev = r.trace_ray_records(kind, rays[:n], hpr)
            assert len(dev) == n and proven_differences(r, tr, scene, two_of(accel), rays[:n], dev, host[:n], f"n={n} kind {kind}") <= SETTLE_CAP
    r.destroy(); tr.close()


def test_host_arrays_cross_the_staging_chunk():
    """n = 2^20 + 65 on the one-triangle scene: two chunks through the staging buffers.  Equal to the same rays sent as two smaller calls, and 4096 rays
    on both sides of the boundary equal the host harness."""
    sc, _ = one_triangle_scene()
    tr, r = TracedScene(sc), renderer(sc, capi.PT_ACCEL_FLAT)
    n = capi.PT_QUERY_CHUNK + 65
    rng = np.random.default_rng(5)
    org = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), np.full((n, 1), 3.0)], 1).astype(np.float32)
    dirs = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
    rays = make_rays(org, dirs, tmax=rng.uniform(3.0, 5.0, n).astype(np.float32), seeds=np.arange(n, dtype=np.uint32))
    big = r.trace_ray_records(NEAREST, rays)
    # (the triangle covers 2 of the 9 square units the rays fall on, and about half of those hits lie inside the ray's range: ~0.11)
    assert 0.05 < ((big["status"] & HIT) != 0).mean() < 0.3 and np.array_equal(big["seed"], rays["seed"])
    k = 600001
    assert records_equal(big, np.concatenate([r.trace_ray_records(NEAREST, rays[:k]), r.trace_ray_records(NEAREST, rays[k:])]))
    lo, hi = capi.PT_QUERY_CHUNK - 2048, capi.PT_QUERY_CHUNK + 2048
    assert records_equal(big[lo:hi], host_query(tr, 0, NEAREST, rays[lo:hi]))
    # CANDIDATES with 16 results per ray: a chunk holds 2^16 rays
    m = capi.PT_QUERY_CHUNK // 16 + 65
    dev = r.trace_ray_records(CANDIDATES, rays[:m], 16)
    assert records_equal(dev, host_query(tr, 0, CANDIDATES, rays[:m], hits_per_ray=16))
    r.destroy(); tr.close()


# ---- device pointers ------------------------------------------------------------------------------------------------------------------------------
def test_device_pointers_from_a_torch_tensor():
    """rays in a torch tensor on the GPU (torch.frombuffer(...).cuda()), results in another: byte for byte the host-pointer call's, for every kind and both
    structures; a pointer offset by 4 bytes is refused with PT_ERR_INVALID.  A process of its own: tests/query_device_child.py says why."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "query_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]


# ---- a query disturbs nothing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("display", [False, True], ids=["plain", "display-images-pending"])
def test_a_query_disturbs_nothing(display):
    env = synth.procedural_sky(128, 64)
    cfg = Config(synth.fuzz_scene(0), env, 64, 48, depth=5)
    tm = hd.default_tonemapper()
    rng = np.random.default_rng(1)
    o = (np.array([0, 0, 6]) + rng.normal(0, 1, (4097, 3))).astype(np.float32)
    rays = make_rays(o, -o / np.linalg.norm(o, axis=1, keepdims=True), seeds=rng.integers(0, 2 ** 32, 4097, dtype=np.uint64).astype(np.uint32))

    def run(query):
        r = renderer(cfg.scene, capi.PT_ACCEL_FLAT)
        integral, _ = r.set_env(cfg.env); r.set_camera(cfg.camera); r.set_sunsky(cfg.sunsky); r.create((cfg.width, cfg.height))
        st = cfg.state(integral)
        images = []
        for f in range(4):
            if f == 2 and query:
                before = r.stats()
                if display:
                    r.tonemap_begin(tm)
                hits = r.trace_ray_records(CLOSEST, rays)
                assert ((hits["status"] & HIT) != 0).mean() > 0.3 and (hits["seed"] != rays["seed"]).any()
                assert r.tonemap_pending() == (2 if display else 0)
                assert r.stats() == before, "pt_Stats across the query"
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


# ---- picker equivalence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_nearest_is_the_picker(accel):
    cfg = Config(synth.fuzz_scene(0), synth.procedural_sky(64, 32), 64, 48)
    r = renderer(cfg.scene, accel)
    picks = [r.pick((i + 0.5) / 8, (j + 0.5) / 8, cfg.camera) for j in range(8) for i in range(8)]
    rays = make_rays([list(p.worldRayOrigin) for p in picks], [list(p.worldRayDirection) for p in picks], seeds=11)
    got = r.trace_ray_records(NEAREST, rays)
    hits = 0
    for p, g in zip(picks, got):
        if p.instanceID == NONE:
            assert g["status"] == 0 and g["instanceID"] == NONE
            continue
        hits += 1
        assert g["status"] == HIT and (g["instanceID"], g["primitiveID"], g["instanceCustomIndex"]) == (p.instanceID, p.primitiveID, p.instanceCustomIndex)
        assert bits(g["t"]) == bits(p.hitT) and bits(g["u"]) == bits(p.baryCoord[1]) and bits(g["v"]) == bits(p.baryCoord[2])
        assert bits(p.baryCoord[0]) == bits(np.float32(1.0) - g["u"] - g["v"])
    assert hits >= 4   # (the comparison above is the test; this only says that the window positions do see the scene)
    r.destroy()


# ---- stack limit ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_stack_limit(accel):
    """camera rays of the spill scene reach the private spill array and equal the host harness; on the overflow scene the call says PT_ERR_STATE with the
    overflow text (a counted condition, as test_overflow_is_reported_everywhere_and_cleared pins it for the other calls) until pt_reset_stats"""
    two = two_of(accel)
    env = synth.procedural_sky(64, 32)
    cfg = Config(synth.deep_chain(synth.DEEP_SPILL_LEVELS), env, 64, 48)
    o, d = deep_rays(cfg)
    rays = make_rays(o, d, seeds=np.arange(len(o), dtype=np.uint32))
    tr, r = TracedScene(cfg.scene), renderer(cfg.scene, accel)
    for kind in (CLOSEST, NEAREST):
        dev = r.trace_ray_records(kind, rays)   # PT_OK
        assert ((dev["status"] & HIT) != 0).mean() > 0.5
        assert proven_differences(r, tr, cfg.scene, two, rays, dev, host_query(tr, two, kind, rays), f"spill scene kind {kind}") <= SETTLE_CAP
    r.destroy(); tr.close()
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), env, 64, 48)
    r = renderer(deep.scene, accel)
    tr = TracedScene(deep.scene)
    away = make_rays([[0, 0, -1e4]], [[0, 0, -1]])   # from behind the camera, away from the chain (which runs along +z for thousands of units): a miss without a walk
    want, over = host_query(tr, two, CLOSEST, away, overflow=True)
    assert over == 0 and want["status"][0] == 0
    tr.close()
    assert records_equal(r.trace_ray_records(CLOSEST, away), want)
    for _ in range(2):
        with pytest.raises(capi.PtError) as e:
            r.trace_ray_records(CLOSEST, rays)
        assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value)
        with pytest.raises(capi.PtError) as e:     # sticky, for every call that hands out results
            r.trace_ray_records(CLOSEST, away)
        assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value)
        with pytest.raises(capi.PtError):
            r.synchronize()
        r.reset_stats()
        r.synchronize()
        assert records_equal(r.trace_ray_records(CLOSEST, away), want)
    r.destroy()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    L = capi.lib()
    sc, _ = one_triangle_scene()
    sc.finalize(capi.pack_vertices)
    rays = make_rays(DEGENERATE_ORG, DEGENERATE_DIR)
    hits = np.zeros((3, 16), hd.rayhit_dtype)
    hits["status"] = 0xABABABAB
    untouched = hits.copy()
    rp, hp = rays.ctypes.data, hits.ctypes.data
    r = HipRenderer(); r.setup(0)
    ctx = r._ctx
    assert L.pt_trace_rays(None, CLOSEST, 0, 3, rp, hp, 1) == capi.PT_ERR_INVALID
    assert L.pt_trace_rays(ctx, CLOSEST, 0, 3, rp, hp, 1) == capi.PT_ERR_STATE              # no scene
    d, keep = sc.desc()
    assert L.pt_set_scene(ctx, C.byref(d)) == capi.PT_OK
    assert L.pt_trace_rays(ctx, CLOSEST, 0, 3, rp, hp, 1) == capi.PT_ERR_STATE              # a scene, no structure
    assert b"pt_build_accel" in L.pt_last_error(ctx)
    assert L.pt_build_accel(ctx) == capi.PT_OK
    bad = [(CLOSEST, 0, 3, None, hp, 1), (CLOSEST, 0, 3, rp, None, 1), (4, 0, 3, rp, hp, 1), (-1, 0, 3, rp, hp, 1), (CLOSEST, 2, 3, rp, hp, 1), (CLOSEST, 0x80000001, 3, rp, hp, 1),
           (CLOSEST, 0, 3, rp, hp, 0), (CLOSEST, 0, 3, rp, hp, 2), (OCCLUDED, 0, 3, rp, hp, 2), (NEAREST, 0, 3, rp, hp, 16), (CANDIDATES, 0, 3, rp, hp, 0), (CANDIDATES, 0, 3, rp, hp, 17),
           (CLOSEST, capi.PT_RAYS_DEVICE, 3, rp + 4, hp, 1), (CLOSEST, capi.PT_RAYS_DEVICE, 3, rp, hp + 4, 1), (CLOSEST, capi.PT_RAYS_DEVICE, 3, rp + 8, hp + 8, 1)]
    assert rp % 16 == 0 and hp % 16 == 0   # (the alignment is checked before anything is launched: host addresses serve as misaligned "device" pointers)
    for args in bad:
        assert L.pt_trace_rays(ctx, *args) == capi.PT_ERR_INVALID, args
        assert L.pt_last_error(ctx).startswith(b"pt_trace_rays")
    assert records_equal(hits, untouched), "a refused call writes nothing"
    assert L.pt_trace_rays(ctx, CLOSEST, 0, 0, None, None, 1) == capi.PT_OK                 # n == 0: nothing to do
    assert L.pt_trace_rays(ctx, CANDIDATES, capi.PT_RAYS_DEVICE, 0, None, None, 16) == capi.PT_OK
    assert records_equal(hits, untouched)
    assert L.pt_trace_rays(ctx, CANDIDATES, 0, 3, rp, hp, 16) == capi.PT_OK and np.array_equal(hits["status"][:, 0], [HIT, HIT, 0])   # no pt_resize needed
    r.destroy()


# ---- C++ shim ---------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_shim_traces_rays(tmp_path):
    """include/pt_renderer.hpp traceRays / traceRaysDevice (device memory from hipMalloc), tests/cpp/query_shim_test.cpp"""
    from tests import shim
    from tests.test_query_host import build_query_shim
    verdict, _ = shim.run(build_query_shim(tmp_path))
    assert verdict == "OK"

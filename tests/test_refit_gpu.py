"""Deforming meshes on the device (pt_update_vertices / pt_refit_accel; csrc/pt_refit.hip): the refitted structure read back and audited node by node
against the DEFORMED vertices (tests/accel_audit.py), held bit for bit to the host build of the same bodies applied to the dump taken before the refit
(tests/refit_host.py), topology and counts unchanged and every box made again; frames and ray queries after deform + refit bit-identical to a second
context that was given the deformed scene and built from it, and to the oracle; sequences of refits; the stale state and every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import accel_audit as A
from tests import refit_host as R
from tests.test_accel_audit_gpu import context, scene
from vk_raytrace_amd import capi

pytestmark = pytest.mark.gpu
U, F = np.uint32, np.float32
SETTINGS = ["build=sahdev,cnodes=1", "build=sahdev,cnodes=0,arena=0", "build=lbvh,cnodes=1"]
MODES = {"flat": ("", True), "two_merged": (",accel=two,mergeSingles=1", True), "two_blas": (",accel=two,mergeSingles=0", False)}
GROUPS = {   # the sizes at which a wave, a block or a single-node tree can go wrong; the degenerate soups and the forest
    "tiny": [f"soup{n}" for n in (1, 2, 3, 4, 5, 13)],
    "wave_block": [f"soup{n}" for n in (63, 64, 65, 257)],
    "large": ["soup2049", "soup5000"],
    "degenerate": ["coincident", "zero_area", "forest"],
}
HOST_ARRAYS = ["WIDE", "TRIS", "ALPHA_RECS", "CNODES", "SHADE_TRIS"]
_deformed = {}


def deformed(name, seed=11, only_mesh=None):
    key = (name, seed, only_mesh)
    if key not in _deformed:
        _deformed[key] = R.deform(scene(name), seed, only_mesh=only_mesh)
    return _deformed[key]


def update(r, new, first=0, count=None):
    count = len(new.vertices) - first if count is None else count
    r.update_vertices(first, new.vertices[first:first + count])


def assert_same_topology(d0, d1):
    for k in ("numTris", "numWideNodes", "nodeCapacity", "numBlas", "mergedTris", "mergedWide", "mergedOnly", "haveCNodes", "haveShadeTris", "numActive"):
        assert d0["info"][k] == d1["info"][k], k
    assert np.array_equal(d0["WIDE"][:, 24:28], d1["WIDE"][:, 24:28])
    assert np.array_equal(d0["TRIS"][:, [3, 7, 11]], d1["TRIS"][:, [3, 7, 11]]) and np.array_equal(d0["ALPHA_RECS"][:, 6:8], d1["ALPHA_RECS"][:, 6:8])
    for k in ("BLAS_RANGES", "MERGED_LIST", "INST_NODE_BASE"):
        assert (d0.get(k) is None) == (d1.get(k) is None) and (d0.get(k) is None or np.array_equal(d0[k], d1[k])), k


def assert_equals_host(d0, d1, S0, S1, what):
    """the dump after the device's refit == the host function applied to the dump before it, on every array the host function returns"""
    want, boxes, costs = R.refit_dump(d0, S0, S1)
    for k in HOST_ARRAYS:
        assert (want.get(k) is None) == (d1.get(k) is None), (what, k)
        if want.get(k) is not None:
            ne = np.nonzero((want[k] != d1[k]).any(1))[0]
            assert len(ne) == 0, f"{what}: {k} differs from the host build in {len(ne)} rows, first {ne[:6].tolist()}"
    if d0["info"]["accelMode"] != 0 and d0["info"]["mergedTris"]:
        assert np.array_equal(want["info"]["mergedBox"].view(U), d1["info"]["mergedBox"].view(U)), what
    return costs


# ---- 1. the audit after the refit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("setting", SETTINGS)
def test_refitted_structure(setting, mode, group):
    extra, merge = MODES[mode]
    with context(setting + extra) as r:
        for name in GROUPS[group]:
            what = f"{setting}{extra} {name}"
            sc = scene(name)
            new, _ = deformed(name)
            S0, S1 = A.scene_inputs(sc, merge_singles=merge), A.scene_inputs(new, merge_singles=merge)
            r.set_scene(sc)
            d0 = A.device_dump(r)
            update(r, new)
            info = r.refit_accel()
            d1 = A.device_dump(r)
            A.assert_clean(A.audit(d1, S1), what)
            assert_same_topology(d0, d1)
            assert R.used_boxes_all_changed(d0, d1) >= len(d0["TRIS"])
            costs = assert_equals_host(d0, d1, S0, S1, what)
            if mode == "flat":
                assert d0["BVH2"] is not None and d1["BVH2"] is None   # the binary nodes are stale after a refit and are released
            for got, want in ((info.costBefore, costs[0]), (info.costAfter, costs[1])):
                assert abs(got - want) <= 1e-9 * want, (what, got, want)
            assert info.slotsWritten == len(d0["TRIS"]) and info.nodesWritten == sum(h.count for k, h in A._hierarchies(d0).items() if k != "tlas")


# ---- 2. a partial update ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", [1, 0])
def test_partial_update_leaves_untouched_meshes_alone(merge):
    sc = scene("forest")
    pm = 5           # the first prim-mesh of 257 triangles: instantiated once (merged when mergeSingles=1)
    pm2 = 4          # 64 triangles, two instances: an object-space BLAS in both settings
    with context(f"build=sahdev,cnodes=1,accel=two,mergeSingles={merge}") as r:
        for mesh in (pm, pm2):
            new, (first, count) = deformed("forest", seed=23, only_mesh=mesh)
            S0, S1 = A.scene_inputs(sc, merge_singles=bool(merge)), A.scene_inputs(new, merge_singles=bool(merge))
            r.set_scene(sc)
            d0 = A.device_dump(r)
            update(r, new, first, count)
            r.refit_accel()
            d1 = A.device_dump(r)
            A.assert_clean(A.audit(d1, S1), f"partial update of prim-mesh {mesh}, mergeSingles={merge}")
            assert_same_topology(d0, d1)
            assert_equals_host(d0, d1, S0, S1, f"partial {mesh}")
            # every BLAS that does not hold the mesh: node range, leaf records and compact nodes bit-identical to before
            ranges, slots = R.tables(d0, S0)
            touched = 0
            for (base, num), (s0, n, form, vo, fi) in zip(ranges[1:] if d0["info"]["mergedTris"] else ranges, slots[1:] if d0["info"]["mergedTris"] else slots):
                assert form == R.RF_VERTEX
                if vo == sc.prim_meshes[mesh][0]:
                    touched += 1
                    assert not np.array_equal(d0["TRIS"][s0:s0 + n], d1["TRIS"][s0:s0 + n])
                    continue
                for k, a, b in (("WIDE", base, base + num), ("CNODES", base, base + num), ("TRIS", s0, s0 + n), ("ALPHA_RECS", s0, s0 + n)):
                    assert np.array_equal(d0[k][a:b], d1[k][a:b]), (mesh, k, base)
            assert touched == (0 if (merge and mesh == pm) else 1)


# ---- 3. / 4. frames and queries -------------------------------------------------------------------------------------------------------------------
def _street():
    from tests.test_two_level import _street as street
    sc = street(60, seed=9)
    sc.finalize(capi.pack_vertices)
    return sc


class Ctx:
    """a context with scene, environment and camera at 64 x 48"""
    W, H, DEPTH = 64, 48, 3

    def __init__(self, sc, env, accel):
        from tests.common import Config
        from vk_raytrace_amd.renderer import HipRenderer
        self.cfg = Config(sc, env, self.W, self.H, depth=self.DEPTH)
        self.r = r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(sc)
        self.integral, _ = r.set_env(self.cfg.env)
        r.set_camera(self.cfg.camera); r.set_sunsky(self.cfg.sunsky); r.create((self.W, self.H))

    def frames(self, n=2, start=0):
        st = self.cfg.state(self.integral)
        for f in range(start, start + n):
            st.frame = f
            self.r.setPushContants(st)
            self.r.run()
        return self.r.read_accum()

    def queries(self, rays):
        o, d, seeds = rays
        out = [self.r.trace_rays(k, o, d, tmax=1.0e4, seeds=seeds) for k in (capi.PT_RAYS_CLOSEST, capi.PT_RAYS_OCCLUDED)]
        return out + [self.r.trace_rays(capi.PT_RAYS_CANDIDATES, o, d, tmax=1.0e4, seeds=seeds, hits_per_ray=4)]


def _rays(n=4096, seed=3):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-25, 25, (n, 3)) * (1, 0.2, 1) + (0, 3, 0)
    t = rng.uniform(-20, 20, (n, 3)) * (1, 0.05, 1)
    return o.astype(F), (t - o).astype(F), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U)


@pytest.fixture(scope="module")
def env_small():
    from vk_raytrace_amd import synth
    return synth.procedural_sky(64, 32)


@pytest.fixture(params=["tail=0", "tail=65536"])
def tail_policy(request):
    import os
    old = os.environ.get("PT_TUNE")
    os.environ["PT_TUNE"] = request.param
    yield request.param
    if old is None:
        os.environ.pop("PT_TUNE", None)
    else:
        os.environ["PT_TUNE"] = old


def _same_records(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL])
def test_frames_and_queries_after_refits_equal_a_fresh_build(env_small, accel, tail_policy):
    """three successive deformations with a refit after each: frames and ray queries equal, bit for bit, those of a second context that was given the
    deformed scene and built its structure from it (the first deformation also against the oracle); then a rebuild on the refitted context is clean, a
    refit with unchanged vertices changes no dumped word, and the reported costs are the auditor's"""
    from tests.common import render_oracle
    from tests.test_gpu_parity import assert_identical
    sc = _street()
    a = Ctx(sc, env_small, accel)
    rays = _rays()
    first = a.frames()
    cur = sc
    try:
        for step in range(3):
            cur, _ = R.deform(cur, seed=40 + step, sigma=0.25)
            update(a.r, cur)
            info = a.r.refit_accel()
            got, got_q = a.frames(), a.queries(rays)
            b = Ctx(cur, env_small, accel)
            try:
                want, want_q = b.frames(), b.queries(rays)
            finally:
                b.r.destroy()
            assert np.array_equal(got.view(U), want.view(U)), f"frames after refit {step}"
            assert _same_records(got_q, want_q), f"queries after refit {step}"
            assert not np.array_equal(got, first)
            assert (got_q[0]["status"] & capi.PT_RAY_HIT).sum() > 500
            if step == 0:
                assert_identical(got, render_oracle(b.cfg, 2), "refitted against the oracle's render of the deformed scene")
            assert info.costBefore > 0 and info.costAfter > info.costBefore * 0.5 and info.ms > 0
        S = A.scene_inputs(cur)
        d1 = A.device_dump(a.r)
        A.assert_clean(A.audit(d1, S), "after three refits")
        built = sum(v for k, v in A.cost(d1).items() if k != "tlas")
        assert abs(info.costAfter - built) <= 1e-9 * built
        # unchanged vertices: update + refit returns every dumped array bit for bit
        update(a.r, cur)
        again = a.r.refit_accel()
        d2 = A.device_dump(a.r)
        for k in A.IDS:
            assert (d1.get(k) is None) == (d2.get(k) is None) and (d1.get(k) is None or np.array_equal(d1[k], d2[k])), k
        assert again.costBefore == info.costBefore and abs(again.costAfter - info.costAfter) <= 1e-12 * info.costAfter
        # a rebuild from the deformed vertices is clean, and costBefore then belongs to the new tree
        a.r._check(a.r._lib.pt_build_accel(a.r._ctx))
        d3 = A.device_dump(a.r)
        A.assert_clean(A.audit(d3, S), "rebuilt after three refits")
        rebuilt = a.r.refit_accel()
        want = sum(v for k, v in A.cost(d3).items() if k != "tlas")
        assert abs(rebuilt.costBefore - want) <= 1e-9 * want and abs(rebuilt.costAfter - want) <= 1e-9 * want
        assert np.array_equal(a.frames().view(U), got.view(U))
    finally:
        a.r.destroy()


# ---- 5. state and refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(fn, code, word=None):
    with pytest.raises(capi.PtError) as e:
        fn()
    assert e.value.code == code, e.value
    assert word is None or word in str(e.value), e.value


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL])
def test_stale_state_and_refusals(env_small, accel):
    from vk_raytrace_amd.renderer import HipRenderer
    sc = _street()
    new, _ = R.deform(sc, seed=61)
    r0 = HipRenderer(); r0.setup(0)
    try:
        _refused(lambda: r0.update_vertices(0, sc.vertices[:4]), capi.PT_ERR_STATE)          # before pt_set_scene
        _refused(r0.refit_accel, capi.PT_ERR_STATE)
        d, keep = sc.desc()
        r0._check(r0._lib.pt_set_scene(r0._ctx, C.byref(d)))
        _refused(r0.refit_accel, capi.PT_ERR_STATE)                                          # a scene, but nothing built
        update(r0, new)                                                                        # without a structure: only the buffer
        r0._check(r0._lib.pt_build_accel(r0._ctx))
        A.assert_clean(A.audit(A.device_dump(r0), A.scene_inputs(new)), "built after an update without a structure")
    finally:
        r0.destroy()
    a = Ctx(sc, env_small, accel)
    r = a.r
    try:
        rays = _rays(256)
        first, q0 = a.frames(), a.queries(rays)
        st = a.cfg.state(a.integral)
        n = len(sc.vertices)
        # refusals that change nothing
        assert r._lib.pt_update_vertices(r._ctx, 0, 4, None) == capi.PT_ERR_INVALID
        assert r._lib.pt_update_vertices(r._ctx, n - 3, 4, new.vertices.ctypes.data) == capi.PT_ERR_INVALID
        assert r._lib.pt_update_vertices(r._ctx, n + 1, 0xFFFFFFFF, new.vertices.ctypes.data) == capi.PT_ERR_INVALID
        assert r._lib.pt_update_vertices(r._ctx, 0xFFFFFFFF, 2, new.vertices.ctypes.data) == capi.PT_ERR_INVALID
        assert r._lib.pt_update_vertices(r._ctx, n, 0, None) == capi.PT_OK and r._lib.pt_update_vertices(r._ctx, 7, 0, None) == capi.PT_OK
        assert np.array_equal(a.frames().view(U), first.view(U)) and _same_records(a.queries(rays), q0)   # not stale, vertex buffer unchanged
        # stale: every call that walks the structure refuses and names the pending refit
        update(r, new)
        walkers = [lambda: (r.setPushContants(st), r.run()), lambda: r.trace_rays(capi.PT_RAYS_CLOSEST, rays[0], rays[1]),
                   lambda: r.trace_paths(st, rays[0], rays[1]), lambda: r.gather_irradiance(st, rays[0][:8], rays[1][:8]), lambda: r.gather_probes(st, rays[0][:8]),
                   lambda: r.pick(0.5, 0.5, a.cfg.camera), lambda: r.capture_guides(), lambda: r.capture_guides_chain(r.guide_chain()), lambda: r.render_instance_plane()]
        for w in walkers:
            _refused(w, capi.PT_ERR_STATE, "refit")
        r.refit_accel()
        for w in walkers:
            w()
        r.synchronize()
        got = a.frames()
        b = Ctx(new, env_small, accel)
        try:
            assert np.array_equal(got.view(U), b.frames().view(U))
        finally:
            b.r.destroy()
        # the three calls that treat a stale structure as built and rebuild it in full
        S = lambda any_hit=True: A.scene_inputs(new, any_hit=any_hit)
        update(r, new)
        r.useAnyHit(False)
        A.assert_clean(A.audit(A.device_dump(r), S(False)), "pt_use_any_hit while stale")
        update(r, new)
        r.useAnyHit(True)
        A.assert_clean(A.audit(A.device_dump(r), S()), "pt_use_any_hit back while stale")
        update(r, new)
        other = capi.PT_ACCEL_TWO_LEVEL if accel == capi.PT_ACCEL_FLAT else capi.PT_ACCEL_FLAT
        r.set_accel_mode(other)
        A.assert_clean(A.audit(A.device_dump(r), S()), "pt_set_accel_mode while stale")
        r.set_accel_mode(accel)
        update(r, new)
        r.update_instances(new)
        A.assert_clean(A.audit(A.device_dump(r), S()), "pt_update_instances while stale")
        assert np.array_equal(a.frames().view(U), got.view(U))
    finally:
        r.destroy()


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL])
def test_refit_of_unchanged_vertices_in_the_middle_of_a_sequence(env_small, accel):
    """4 frames == 2 frames, update + refit with the vertices the scene has, 2 more frames: the running mean and the sample counters go on"""
    sc = _street()
    a, b = Ctx(sc, env_small, accel), Ctx(sc, env_small, accel)
    try:
        want = a.frames(4)
        b.frames(2)
        update(b.r, sc)
        b.r.refit_accel()
        got = b.frames(2, start=2)
        assert np.array_equal(got.view(U), want.view(U))
        sa, sb = a.r.stats(), b.r.stats()
        for k in ("samples", "closestRays", "shadowRays", "shadedHits", "misses", "alphaTests", "neeLookups", "numTriangles"):
            assert sa[k] == sb[k], k
    finally:
        a.r.destroy(); b.r.destroy()


def test_cost_before_survives_a_rebuild_of_the_merged_structure_alone():
    """two-level: after a refit, pt_update_instances of a once-instantiated node builds the merged structure again (new topology, new parent table).
    costBefore of the next refit is then the cost of the BLASes as pt_build_accel left them -- not as the earlier refit deformed them -- plus the
    cost of the merged structure as it was just built"""
    import copy
    from vk_raytrace_amd.scene import translate
    sc = scene("forest")
    new, _ = deformed("forest")
    with context("build=sahdev,cnodes=1,accel=two,mergeSingles=1") as r:
        r.set_scene(sc)
        built = A.cost(A.device_dump(r))
        update(r, new)
        first = r.refit_accel()
        want0 = sum(v for k, v in built.items() if k != "tlas")
        assert abs(first.costBefore - want0) <= 1e-9 * want0 and abs(first.costAfter - first.costBefore) > 1e-6 * want0   # (continuous offsets: the cost moved)
        moved = copy.copy(new)
        moved.nodes = list(new.nodes)
        m0, p0 = moved.nodes[0]
        assert sum(1 for _, p in moved.nodes if p == p0) == 1   # instantiated once: it lives in the merged structure
        moved.nodes[0] = (translate(0.5, -0.25, 1.0) @ m0, p0)
        r.update_instances(moved)
        d2 = A.device_dump(r)
        A.assert_clean(A.audit(d2, A.scene_inputs(moved)), "after moving a merged instance of the refitted structure")
        now = A.cost(d2)
        info = r.refit_accel()
        want = now["merged"] + sum(v for k, v in built.items() if k.startswith("blas"))
        assert abs(info.costBefore - want) <= 1e-9 * want, (info.costBefore, want)
        stale = sum(v for k, v in now.items() if k != "tlas")   # what measuring everything again would have reported
        assert abs(info.costAfter - stale) <= 1e-9 * stale and abs(stale - want) > 1e-6 * want   # (the two readings differ: the test tells them apart)

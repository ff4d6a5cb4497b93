"""pt_trace_rays' per-ray body on the CPU: vk_raytrace_amd/csrc/pt_query.h (query_ray<TWO>, what the query kernel runs per lane) compiled for the
host by tests/cpp/query_host.cpp, a unit of the host harness (tests/host_harness.py: qh_query), and held ray by ray to the definitions that harness
already has:

  PT_RAYS_CLOSEST / PT_RAYS_OCCLUDED  th_settle's exact key-ordered loop (trace contract T5 / T6): hit, barycentrics AND the RNG state afterwards
  PT_RAYS_CANDIDATES                  th_candidates mode 0, brute force over every world triangle, by compare()'s rule of tests/host_harness.py
  PT_RAYS_NEAREST                     the same brute force with TRI_NOCULL forced on every instance (the picker's flag-less ray)

Scenes, rays and rules are the harness's, the ones tests/test_trace_host.py uses.  tests/test_query_gpu.py runs the same rays through the C ABI on the device and compares them, record
by record, with what this harness returns (the helpers below are shared with it)."""

import numpy as np
import pytest

from tests import shim
from tests.host_harness import NONE, NOCULL, OPAQUE, Traced, TracedScene, accidental_differences, alpha_scenes, instanced_scene, rays_for, scene_rays
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.scene import Scene, translate, rotate_y

CLOSEST, OCCLUDED, NEAREST, CANDIDATES = capi.PT_RAYS_CLOSEST, capi.PT_RAYS_OCCLUDED, capi.PT_RAYS_NEAREST, capi.PT_RAYS_CANDIDATES
HIT, INVALID = capi.PT_RAY_HIT, capi.PT_RAY_INVALID
INF = np.float32(1e32)  # PT_INFINITY: what th_candidates / th_settle take for "unbounded"
ACCIDENTAL_CAP = 12     # test_walks_report_brute_force_candidates gives this cap to the host walks on the same rays (see test_candidates_equal_brute_force for what it sees)


def make_rays(org, dirs, tmax=None, seeds=None):
    org = np.asarray(org, np.float32).reshape(-1, 3)
    rays = np.zeros(len(org), hd.ray_dtype)
    rays["origin"], rays["direction"] = org, np.asarray(dirs, np.float32).reshape(-1, 3)
    rays["tmax"] = INF if tmax is None else np.asarray(tmax, np.float32)
    rays["seed"] = 0 if seeds is None else np.asarray(seeds, np.uint32)
    return rays


def host_query(tr, two, kind, rays, variant=0, hits_per_ray=1, overflow=False):
    """query_ray on the host; returns (n,) records, (n, hits_per_ray) for CANDIDATES.  overflow: also return the traversal-stack overflows"""
    rays = np.ascontiguousarray(rays, hd.ray_dtype)
    hits = np.zeros((len(rays), hits_per_ray), hd.rayhit_dtype)
    over = tr.L.qh_query(tr.h, int(two), int(kind), int(variant), len(rays), rays.ctypes.data, hits.ctypes.data, hits_per_ray)
    out = hits if kind == CANDIDATES else hits[:, 0]
    if overflow:
        return out, over
    assert over == 0, "traversal stack overflow"
    return out


def tri_base(scene):
    """world index of every node's first triangle, from the scene description: nodes in order, each with its prim-mesh's triangles"""
    counts = [scene.prim_meshes[pm][3] // 3 for _, pm in scene.nodes]
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if counts else np.zeros(0, np.int64)


def world_index(scene, hits):
    """(instanceID, primitiveID) -> world triangle index (NONE on a miss); also checks the record's own consistency"""
    hit = (hits["status"] & HIT) != 0
    base = tri_base(scene)
    pms = np.array([pm for _, pm in scene.nodes], np.int64)
    inst = hits["instanceID"].astype(np.int64)
    assert (inst[hit] < len(base)).all() and (hits["primitiveID"][hit] >= 0).all()
    assert (hits["instanceID"][~hit] == NONE).all() and (hits["primitiveID"][~hit] == -1).all() and (hits["instanceCustomIndex"][~hit] == -1).all()
    assert (hits["t"][~hit] == 0).all() and (hits["u"][~hit] == 0).all() and (hits["v"][~hit] == 0).all()
    w = np.full(hits.shape, NONE, np.int64)
    w[hit] = base[inst[hit]] + hits["primitiveID"][hit]
    assert (hits["instanceCustomIndex"][hit] == pms[inst[hit]]).all(), "instanceCustomIndex is the node's prim-mesh"
    return w.astype(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def records_equal(a, b):
    """every field of every record, floats by their bits"""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def alpha_inputs(tr, eye, spread, n=6000):
    """the rays, seeds and shadow ranges of test_two_pass_alpha_equals_the_key_ordered_loop (same generator, same order of draws)"""
    rng = np.random.default_rng(4242)
    org, dirs = scene_rays(tr, rng, n, eye, spread)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    tmax = np.where(rng.random(n) < 0.3, np.float32(1e32), rng.uniform(0.3, 12.0, n)).astype(np.float32)
    return org, dirs, seeds, tmax


# ---- alpha scenes: CLOSEST and OCCLUDED against the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scene,eye,spread", list(alpha_scenes()), ids=lambda x: x if isinstance(x, str) else None)
def test_closest_and_occluded_equal_the_key_ordered_loop(name, scene, eye, spread):
    """On exactly the inputs on which the existing test finds zero differences among the host legs: every ray's t, u, v (bits), world triangle and
    seed equal th_settle(exact = 1) on the flat structure -- for both structures; the shadow verdict and seed for both variants."""
    tr = TracedScene(scene)
    org, dirs, seeds, tmax = alpha_inputs(tr, eye, spread)
    ref_w, ref_tuv, ref_seed, ref_draws = tr.settle(0, 0, 1, org, dirs, seeds)
    assert (ref_w != NONE).mean() > 0.5 and ref_draws.sum() > len(org) // 20 and (ref_seed != seeds).any(), "the scene must exercise hits and alpha draws"
    # (scene_rays sends a ray between two surface points that may coincide: its zero direction is the one invalid ray of these inputs -- reported as
    # such, and otherwise what the definition makes of it: a miss with the seed untouched)
    invalid = np.where((dirs == 0).all(1), np.uint32(INVALID), np.uint32(0))
    assert invalid.sum() <= 2 * INVALID
    rays = make_rays(org, dirs, tmax=0.25, seeds=seeds)   # CLOSEST ignores tmax: a bound in front of most hits must change nothing
    for two in (0, 1):
        got = host_query(tr, two, CLOSEST, rays)
        w = world_index(scene, got)                        # (instanceID, primitiveID) names the world triangle
        hit = ref_w != NONE
        differ = (w != ref_w) | (got["seed"] != ref_seed) | ((got["status"] & ~np.uint32(HIT)) != invalid) | (hit & ((bits(got["t"]) != bits(ref_tuv[:, 0])) | (bits(got["u"]) != bits(ref_tuv[:, 1])) | (bits(got["v"]) != bits(ref_tuv[:, 2]))))
        assert not differ.any(), f"{name}: CLOSEST two={two}: {np.count_nonzero(differ)} rays differ, first {np.nonzero(differ)[0][:5]}"
    rays = make_rays(org, dirs, tmax=tmax, seeds=seeds)
    for variant in (capi.PT_VARIANT_RAYQUERY, capi.PT_VARIANT_RTX):
        want_w, _, want_seed, _ = tr.settle(1, 0, 1, org, dirs, seeds, tmax, variant)
        assert 0.05 < want_w.mean() < 0.95
        for two in (0, 1):
            got = host_query(tr, two, OCCLUDED, rays, variant=variant)
            differ = ((got["status"] & HIT) != want_w) | (got["seed"] != want_seed) | ((got["status"] & ~np.uint32(HIT)) != invalid)
            assert not differ.any(), f"{name}: OCCLUDED variant={variant} two={two}: {np.count_nonzero(differ)} rays differ"
            assert (got["instanceID"] == NONE).all() and (got["t"] == 0).all() and (got["primitiveID"] == -1).all()   # no hit fields
        if variant == capi.PT_VARIANT_RTX:
            assert np.array_equal(want_seed, seeds)
    tr.close()


# ---- instanced scenes: CANDIDATES and NEAREST against brute force ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 3])
def test_candidates_equal_brute_force(seed):
    """Counts of accidental hits that test_walks_report_brute_force_candidates sees for its host walks on these rays (both structures together,
    measured when this test was written): scene 0: none on either structure; scene 3: 2 rays on the flat and 2 on the two-level structure, 4 in its
    count.  The cap is that test's: 12 -- here per structure."""
    sc, flags, off = instanced_scene(seed)
    tr = Traced(sc, flags)
    org, dirs = rays_for(tr, np.random.default_rng(100 + seed), off, 6000)
    ref_w, ref_t = tr.candidates(0, org, dirs, max_cand=6)
    assert (ref_w != NONE).sum() > 8000
    rays = make_rays(org, dirs, seeds=np.arange(len(org)))
    for two in (0, 1):
        got = host_query(tr, two, CANDIDATES, rays, hits_per_ray=6)
        assert (got["seed"] == rays["seed"][:, None]).all() and ((got["status"] & ~np.uint32(HIT)) == 0).all()
        n = accidental_differences(tr, org, dirs, ref_w, ref_t, world_index(sc, got), got["t"], f"scene {seed} two={two}")
        print(f"CANDIDATES scene {seed} two={two}: {n} rays differ from brute force through an ill-conditioned candidate")
        assert n <= ACCIDENTAL_CAP, n
    tr.close()


@pytest.mark.parametrize("seed", [0, 3])
def test_nearest_ignores_culling(seed):
    """instanced_scene mixes culled (even nodes) and double-sided instances; the picker's ray counts every triangle: brute force over the same
    geometry with TRI_NOCULL forced on every instance, nearest key inside (0, tmax), unbounded and bounded"""
    sc, flags, off = instanced_scene(seed)
    assert (flags & NOCULL).any() and not (flags & NOCULL).all()
    tr = Traced(sc, flags)
    brute = Traced(sc, flags | NOCULL)
    org, dirs = rays_for(tr, np.random.default_rng(100 + seed), off, 6000)
    culled_w, _ = tr.candidates(0, org, dirs, max_cand=1)
    for tmax in (INF, np.float32(9.0)):
        ref_w, ref_t = brute.candidates(0, org, dirs, tmax=float(tmax), max_cand=1)
        if tmax == INF:
            assert (ref_w != culled_w).mean() > 0.05, "culling must matter on these rays"
        rays = make_rays(org, dirs, tmax=tmax, seeds=7)
        for two in (0, 1):
            got = host_query(tr, two, NEAREST, rays)
            assert (got["seed"] == 7).all()
            n = accidental_differences(brute, org, dirs, ref_w, ref_t, world_index(sc, got)[:, None], got["t"][:, None], f"NEAREST scene {seed} two={two} tmax={tmax}")
            assert n <= ACCIDENTAL_CAP, n
            assert (got["t"][(got["status"] & HIT) != 0] < tmax).all()
    tr.close(); brute.close()


# ---- edges ------------------------------------------------------------------------------------------------------------------------------------
def one_triangle_scene():
    sc = Scene("one")
    m = sc.add_material()
    sc.add_node(sc.add_prim_mesh([(-1, -1, 0), (1, -1, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [(0, 0), (1, 0), (0.5, 1)], [0, 1, 2], m), translate(0.2, 0.1, -1.0) @ rotate_y(0.4))
    return sc, [OPAQUE | NOCULL]


def empty_scenes():
    empty = Scene("empty")
    m = empty.add_material()
    hole = empty.add_prim_mesh(np.zeros((3, 3)), [(0, 0, 1)] * 3, np.zeros((3, 2)), np.zeros(0, np.uint32), m)
    empty.add_node(hole); empty.add_node(hole, translate(1, 2, 3))
    yield empty, [OPAQUE, OPAQUE]


def three_layer_scene():
    """three instances of one triangle stacked along z: a ray down the z axis has exactly three candidates"""
    sc = Scene("layers")
    m = sc.add_material()
    pm = sc.add_prim_mesh([(-1, -1, 0), (1, -1, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [(0, 0), (1, 0), (0.5, 1)], [0, 1, 2], m)
    for z in (0.0, -1.0, -2.5):
        sc.add_node(pm, translate(0, 0, z))
    return sc, [OPAQUE | NOCULL] * 3


DEGENERATE_ORG = np.array([[0, 0, 3], [0.2, 0.1, 3], [5, 5, 5]], np.float32)   # the rays of test_degenerate_inputs
DEGENERATE_DIR = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1]], np.float32)
ALL_KINDS = (CLOSEST, OCCLUDED, NEAREST, CANDIDATES)


def test_degenerate_scenes():
    sc, flags = one_triangle_scene()
    tr = Traced(sc, flags)
    ref_w, ref_t = tr.candidates(0, DEGENERATE_ORG, DEGENERATE_DIR, max_cand=1)
    assert (ref_w[:2, 0] == 0).all() and ref_w[2, 0] == NONE
    rays = make_rays(DEGENERATE_ORG, DEGENERATE_DIR, seeds=[5, 6, 7])
    for two in (0, 1):
        for kind in (CLOSEST, NEAREST, CANDIDATES):
            got = host_query(tr, two, kind, rays).reshape(3)
            assert np.array_equal(world_index(sc, got), ref_w[:, 0]) and np.array_equal(bits(got["t"]), bits(ref_t[:, 0])) and np.array_equal(got["seed"], [5, 6, 7])
            assert np.array_equal(got["status"], [HIT, HIT, 0]) and (got["u"][:2] > 0).all() and (got["u"][:2] + got["v"][:2] < 1).all()
        got = host_query(tr, two, OCCLUDED, rays)
        assert np.array_equal(got["status"], [HIT, HIT, 0]) and (world_index(sc, got[2:]) == NONE).all() and (got["instanceID"] == NONE).all()
    tr.close()
    for sc, flags in empty_scenes():
        tr = Traced(sc, flags)
        for two in (0, 1):
            for kind in ALL_KINDS:
                got = host_query(tr, two, kind, rays)
                assert (got["status"] == 0).all() and (world_index(sc, got) == NONE).all() and (got["seed"].reshape(3, -1) == rays["seed"][:, None]).all()
        tr.close()


def test_the_upper_bound_is_exclusive_and_an_empty_range_is_a_miss():
    sc, flags = one_triangle_scene()
    tr = Traced(sc, flags)
    t_hit = tr.candidates(0, DEGENERATE_ORG[:1], DEGENERATE_DIR[:1], max_cand=1)[1][0, 0]
    assert t_hit > 0
    tm = np.array([t_hit, np.nextafter(t_hit, np.float32(np.inf)), 0.0, -1.0, -np.inf, np.inf], np.float32)
    rays = make_rays(np.repeat(DEGENERATE_ORG[:1], len(tm), 0), np.repeat(DEGENERATE_DIR[:1], len(tm), 0), tmax=tm, seeds=3)
    for two in (0, 1):
        for kind in (OCCLUDED, NEAREST, CANDIDATES):
            got = host_query(tr, two, kind, rays).reshape(len(tm))
            assert np.array_equal(got["status"], [0, HIT, 0, 0, 0, HIT]), (two, kind, got["status"])   # tmax == t: outside; plain misses, never INVALID
            if kind != OCCLUDED:
                assert (world_index(sc, got) == np.where(got["status"] == HIT, 0, NONE)).all()
        got = host_query(tr, two, CLOSEST, rays)           # unbounded: tmax is ignored
        assert (got["status"] == HIT).all() and (bits(got["t"]) == bits(t_hit)).all()
    tr.close()


def invalid_ray_cases():
    """one ray per rule: (origin, direction, tmax, kinds for which it is invalid)"""
    o, d = DEGENERATE_ORG[0], DEGENERATE_DIR[0]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    yield "NaN origin component", (o[0], nan, o[2]), d, INF, ALL_KINDS
    yield "+Inf direction component", o, (inf, 0, -1), INF, ALL_KINDS
    yield "-Inf origin component", (o[0], o[1], -inf), d, INF, ALL_KINDS
    yield "NaN direction component", o, (0, 0, nan), INF, ALL_KINDS
    yield "zero direction", o, (0, -0.0, 0), INF, ALL_KINDS
    yield "NaN tmax", o, d, nan, (OCCLUDED, NEAREST, CANDIDATES)   # CLOSEST ignores tmax: the ray is valid there


def invalid_ray_batch():
    """the invalid rays with valid neighbours on both sides: rays, index of every invalid one, the kinds it is invalid for"""
    cases = list(invalid_ray_cases())
    org, dirs, tm, where = [], [], [], []
    for i, (_, o, d, t, kinds) in enumerate(cases):
        org += [DEGENERATE_ORG[i % 3], o]; dirs += [DEGENERATE_DIR[i % 3], d]; tm += [INF, t]
        where.append((2 * i + 1, kinds))
    org.append(DEGENERATE_ORG[1]); dirs.append(DEGENERATE_DIR[1]); tm.append(INF)
    return make_rays(np.array(org, np.float32), np.array(dirs, np.float32), tmax=np.array(tm, np.float32), seeds=100 + np.arange(len(org))), where


def test_invalid_rays_are_reported_per_ray():
    sc, flags = one_triangle_scene()
    tr = Traced(sc, flags)
    rays, where = invalid_ray_batch()
    for two in (0, 1):
        for kind in ALL_KINDS:
            hpr = 2 if kind == CANDIDATES else 1
            got = host_query(tr, two, kind, rays, hits_per_ray=hpr).reshape(len(rays), hpr)
            bad = np.array([i for i, kinds in where if kind in kinds])
            good = np.setdiff1d(np.arange(len(rays)), bad)
            assert (got["status"][bad] == INVALID).all(), (two, kind, got["status"][:, 0])
            assert (got["seed"][bad] == rays["seed"][bad][:, None]).all() and (world_index(sc, got[bad]) == NONE).all()
            alone = host_query(tr, two, kind, rays[good], hits_per_ray=hpr).reshape(len(good), hpr)
            assert records_equal(got[good], alone) and ((got["status"][good] & INVALID) == 0).all()   # the neighbours are unaffected
            assert (got["status"][good][:, 0] == HIT).sum() >= 4
    tr.close()


def test_sixteen_results_for_a_ray_with_three_candidates():
    sc, flags = three_layer_scene()
    tr = Traced(sc, flags)
    rays = make_rays([[0, -0.2, 5]], [[0, 0, -1]], seeds=9)
    for two in (0, 1):
        got = host_query(tr, two, CANDIDATES, rays, hits_per_ray=16)[0]
        assert np.array_equal(got["status"], [HIT] * 3 + [0] * 13) and np.array_equal(got["instanceID"][:3], [0, 1, 2]) and (got["seed"] == 9).all()
        assert np.array_equal(got["t"][:3], np.array([5.0, 6.0, 7.5], np.float32)) and (world_index(sc, got[3:]) == NONE).all()
        one = host_query(tr, two, CANDIDATES, rays, hits_per_ray=2)[0]
        assert records_equal(one, got[:2])
    tr.close()


# ---- C++ shim -----------------------------------------------------------------------------------------------------------------------------------
def build_query_shim(tmp_path):
    return shim.build_shim(tmp_path, "query_shim_test", ("-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include"))   # (the program calls hipMalloc itself)


def test_cpp_shim_with_ray_queries_builds_and_fails_loudly_without_gpu(tmp_path):
    """in the style of tests/test_cpp_shim.py: the shim's traceRays / traceRaysDevice compile against the C ABI and link; without a device setup() says so"""
    verdict, _ = shim.run(build_query_shim(tmp_path))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")

"""The product's traversal source on the CPU: vk_raytrace_amd/csrc/pt_trace.h (traverse<MODE, TWO>, the fused slab test, the two-level
walk with its per-instance box padding, tri_test) compiled for the host by tests/cpp/trace_host.cpp and held, ray by ray, to a brute-force
loop over every world triangle with the same triangle test.

Claim under test ("trace contract"): the walk reports exactly the candidates brute force reports -- every triangle T2
accepts along the ray, in key order (t, world index) -- for the flat structure and for the two-level structure, on instanced scenes with
scaled / rotated / mirrored / far-translated instances, for camera rays, rays between surface points (bounce rays start a few ulps off a
surface), axis-parallel rays and rays from far outside the scene.  A candidate on which a walk and brute force disagree is acceptable only
if fp32's verdict on one of the triangles involved is an artefact of cancellation: an ACCIDENTAL hit (Moeller-Trumbore accepting a triangle
the ray misses in double precision) or a hit distance that is off by more than the box tolerance (nearly edge-on triangle) -- such a
candidate is found or not depending on the shape of the boxes around it and on the order of the walk (DESIGN.md section 3 documents the
one case seen on the GPU).  Even the flat walk differs from brute force in such cases; what must never happen is a walk losing a
well-conditioned hit.

The harness itself -- its build, its table of entry points, Traced / TracedScene / host_render, the scenes and the rays -- is tests/host_harness.py.
"""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import host_harness
from tests.host_harness import NONE, NOCULL, OPAQUE, Traced, TracedScene, alpha_scenes, compare, deep_rays, host_render, instanced_scene, rays_for, scene_rays
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.scene import Scene, translate, rotate_y


@pytest.mark.parametrize("seed,merge", [(0, True), (1, True), (2, True), (3, True), (0, False), (3, False)])
def test_walks_report_brute_force_candidates(seed, merge):
    sc, flags, off = instanced_scene(seed)
    tr = Traced(sc, flags, merge_singles=merge)
    rng = np.random.default_rng(100 + seed)
    org, dirs = rays_for(tr, rng, off, 6000)
    total, accidental = compare(tr, org, dirs, f"scene {seed}")
    assert total > 8000                       # the rays do hit things (several candidates each)
    # Every disagreement was verified to be an accidental hit (compare()).  They are not rare HERE because a quarter of the rays start thousands
    # of units away, where |o - p0| ~ 5e3 leaves fp32 only ~1e-3 of absolute resolution in Moeller-Trumbore's numerators (brute force then reports
    # hits at t = 4096.0 exactly and the like; both walks, flat and two-level, never get near those triangles).  On the GPU workloads
    # (camera inside the scene) the rate is ~1e-8 per ray.  A hole in the box tests would show up as hundreds of GENUINE misses, not as these.
    assert accidental <= 12, accidental
    nflat, nblas, ntlas, nslots = tr.sizes()
    assert nblas < nflat and nslots < tr.n    # meshes are stored once in the two-level structure
    tr.close()


def test_far_from_the_origin_and_shadow_range():
    """instances around (3000, -1500, 800): fp32 resolution there is 2.4e-4, the object-space padding must absorb the rounding of the ray
    transform; bounded rays (tmax) prune the same candidates on all sides"""
    sc, flags, off = instanced_scene(11, n_nodes=90, far=True)
    tr = Traced(sc, flags)
    rng = np.random.default_rng(7)
    org, dirs = rays_for(tr, rng, off, 4000)
    total, accidental = compare(tr, org, dirs, "far scene")
    assert total > 4000 and accidental <= 12, (total, accidental)
    ref_w, ref_t = tr.candidates(0, org[:1500], dirs[:1500], tmax=9.0)
    for mode in (1, 2):
        w, t = tr.candidates(mode, org[:1500], dirs[:1500], tmax=9.0)
        same = (w == ref_w).all(1) & (t.view(np.uint32) == ref_t.view(np.uint32)).all(1)
        assert same.mean() > 0.999
        assert (ref_t[ref_w != NONE] < 9.0).all()
    tr.close()


def test_degenerate_inputs():
    """one triangle in one instance (single-leaf BLAS and TLAS), an empty scene, a scene of empty instances"""
    sc = Scene("one")
    m = sc.add_material()
    sc.add_node(sc.add_prim_mesh([(-1, -1, 0), (1, -1, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [(0, 0), (1, 0), (0.5, 1)], [0, 1, 2], m), translate(0.2, 0.1, -1.0) @ rotate_y(0.4))
    tr = Traced(sc, [OPAQUE | NOCULL])
    org = np.array([[0, 0, 3], [0.2, 0.1, 3], [5, 5, 5]], np.float32)
    dirs = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1]], np.float32)
    ref = tr.candidates(0, org, dirs)
    for mode in (1, 2):
        got = tr.candidates(mode, org, dirs)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    assert (ref[0][:2, 0] == 0).all() and ref[0][2, 0] == NONE
    tr.close()
    empty = Scene("empty")
    m = empty.add_material()
    hole = empty.add_prim_mesh(np.zeros((3, 3)), [(0, 0, 1)] * 3, np.zeros((3, 2)), np.zeros(0, np.uint32), m)
    empty.add_node(hole); empty.add_node(hole, translate(1, 2, 3))
    tr = Traced(empty, [OPAQUE, OPAQUE])
    for mode in (0, 1, 2):
        assert (tr.candidates(mode, org, dirs)[0] == NONE).all()
    tr.close()


# ---- stochastic alpha: the product's two-pass settle functions against the contract's key-ordered loop -------------------------------------
@pytest.mark.parametrize("name,scene,eye,spread", list(alpha_scenes()), ids=lambda x: x if isinstance(x, str) else None)
def test_two_pass_alpha_equals_the_key_ordered_loop(name, scene, eye, spread):
    """trace contract T5 / T6 with stochastic alpha: the product's settle functions (pass A nearest certain hit, pass B count of the zero-
    opacity candidates in front of it, draws consumed in bulk, exact fallback; opacity maps answering most evaluations) -- in the lock-step
    form k_tail and the k_*_s kernels use (traverse<>) and in the resumable per-lane form of the persistent kernels (pt_machine.h) -- must return the hit,
    the barycentrics AND the RNG state of the definition -- candidates strictly in key order, one draw per non-opaque candidate -- on the flat
    and on the two-level structure, for closest-hit rays, bounded shadow rays and the RT-pipeline flavour of the shadow ray."""
    tr = TracedScene(scene)
    rng = np.random.default_rng(4242)
    n = 6000
    org, dirs = scene_rays(tr, rng, n, eye, spread)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    ref = tr.settle(0, 0, 1, org, dirs, seeds)                      # the definition, flat structure
    assert (ref[0] != NONE).mean() > 0.5 and ref[3].sum() > n // 20, "the scene must exercise hits and alpha draws"
    for two, exact in ((0, 0), (1, 0), (1, 1), (0, 2), (1, 2)):   # exact = 2: the trace machine of the persistent kernels (pt_machine.h)
        got = tr.settle(0, two, exact, org, dirs, seeds)
        same = (got[0] == ref[0]) & (got[1].view(np.uint32) == ref[1].view(np.uint32)).all(1) & (got[2] == ref[2])
        # (a ray may differ only through an ill-conditioned candidate, see test_walks_report_brute_force_candidates: none is expected at this size)
        assert same.all(), f"{name}: closest-hit, two={two} exact={exact}: {np.count_nonzero(~same)} rays differ, first {np.nonzero(~same)[0][:5]}"
        if exact != 1:
            assert np.array_equal(got[3], ref[3])                   # the alpha-test counter (pt_Stats.alphaTests) counts the same draws
    # the persistent kernels on the compact form of the flat structure's nodes (PT_TUNE cnodes=1: 80-byte nodes, fp16 grid planes): the boxes are
    # looser, never tighter -- same hits, barycentrics, RNG states and draw counts
    trc = TracedScene(scene, compact_nodes=True)
    assert trc.L.th_compact_ok(trc.h) == 1
    for two in (0, 1):
        got = trc.settle(0, two, 2, org, dirs, seeds)
        same = (got[0] == ref[0]) & (got[1].view(np.uint32) == ref[1].view(np.uint32)).all(1) & (got[2] == ref[2])
        assert same.all(), f"{name}: closest-hit on compact nodes, two={two}: {np.count_nonzero(~same)} rays differ, first {np.nonzero(~same)[0][:5]}"
        assert np.array_equal(got[3], ref[3])
    tmax = np.where(rng.random(n) < 0.3, np.float32(1e32), rng.uniform(0.3, 12.0, n)).astype(np.float32)
    # ... and bounded shadow rays on them (the machine's loop as k_trace_p / k_closest_p / k_shadow_p drive it: lane_inner, then lane_leaf)
    for variant in (0, 1):
        want = tr.settle(1, 0, 1, org, dirs, seeds, tmax, variant)
        got = trc.settle(1, 0, 2, org, dirs, seeds, tmax, variant)
        assert (got[0] == want[0]).all() and (got[2] == want[2]).all(), f"{name}: shadow rays on compact nodes, variant={variant}"
    trc.close()
    for variant in (0, 1):
        ref = tr.settle(1, 0, 1, org, dirs, seeds, tmax, variant)
        for two, exact in ((0, 0), (1, 0), (1, 1), (0, 2), (1, 2)):
            got = tr.settle(1, two, exact, org, dirs, seeds, tmax, variant)
            same = (got[0] == ref[0]) & (got[2] == ref[2])
            assert same.all(), f"{name}: shadow variant {variant}, two={two} exact={exact}: {np.count_nonzero(~same)} rays differ"
        if variant == 1:
            assert np.array_equal(ref[2], seeds)                    # RT pipeline: the any-hit shader draws from a copy of the seed
    tr.close()


@pytest.mark.parametrize("far", [False, True])
def test_compact_nodes_never_lose_a_hit(far):
    """The 80-byte form of the nodes (pt_cnode.h cn_encode, pt_trace.h wide_node_step_c) on the adversarial instanced scene -- scales 0.2 .. 5, mirrored
    and coincident instances, rays that start thousands of units away (far=True: every coordinate carries an offset of thousands, the worst case
    for the per-node grid's p * idir + n): the persistent kernels' walk on compact nodes returns the hits of the walk on the fp32 nodes."""
    sc, flags, off = instanced_scene(11, far=far)
    tr = TracedScene(sc)
    trc = TracedScene(sc, compact_nodes=True)
    assert trc.L.th_compact_ok(trc.h) == 1
    rng = np.random.default_rng(5)
    org, dirs = rays_for(tr, rng, off, 8000)
    seeds = np.zeros(len(org), np.uint32)
    # the property itself, plane by plane in double: every decoded box encloses the fp32 box it stands for, the child references are the same
    loose = C.c_double()
    assert trc.L.th_cnode_violations(trc.h, C.byref(loose)) == 0
    assert 0.0 <= loose.value <= 2.0 / 2047, loose.value  # and by at most one grid step per plane (mean growth of a child's extent, in units of the node's grid extent)
    for two in (0, 1):   # flat structure; two-level structure (TLAS + object-space BLASes with their per-instance padding + the merged structure)
        assert trc.L.th_compact_in_use(trc.h, two) == 1 and tr.L.th_compact_in_use(tr.h, two) == 0
        want = tr.settle(0, two, 2, org, dirs, seeds)
        got = trc.settle(0, two, 2, org, dirs, seeds)
        assert (want[0] != NONE).mean() > 0.3
        same = (got[0] == want[0]) & (got[1].view(np.uint32) == want[1].view(np.uint32)).all(1)
        assert same.all(), f"two={two}: {np.count_nonzero(~same)} rays differ, first {np.nonzero(~same)[0][:5]}"
    tr.close(); trc.close()


# ---- whole frames: the product's shading source on the host against the oracle ---------------------------------------------------------------
def _bits_equal(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(np.where(an, 0, a).view(np.uint32), np.where(bn, 0, b).view(np.uint32))


@pytest.mark.parametrize("two", [0, 1])
def test_host_build_of_the_shading_source_renders_the_oracles_frames(two):
    """End to end without a GPU: camera ray, traversal with stochastic alpha, shading state, materials and textures, environment NEE through the
    alias table, both BSDFs, punctual lights, sun & sky, Russian roulette, firefly clamp and the running mean -- the functions the HIP kernels
    are made of, compiled by g++ -- give the CPU oracle's accumulation images BIT FOR BIT (the oracle is in turn bit-identical to the
    reference's own shaders, tests/test_oracle_vs_ref.py).  On the GPU the same comparison is tests/test_gpu_parity.py."""
    from tests.common import Config, render_oracle
    env = synth.procedural_sky(128, 64)
    # every material feature + punctual lights, both BSDFs, several samples per frame
    for pbr in (0, 1):
        cfg = Config(synth.feature_box(tex_size=32, lights=True), env, 64, 48, depth=6, pbr=pbr, max_samples=2)
        assert _bits_equal(host_render(cfg, 2, two), render_oracle(cfg, 2)), ("feature box", pbr)
    # first-hit AOVs
    for mode in (hd.eNormal, hd.eTexcoord, hd.eBaseColor, hd.eAlpha):
        cfg = Config(synth.feature_box(tex_size=32), env, 64, 48, debug=mode)
        assert _bits_equal(host_render(cfg, 1, two), render_oracle(cfg, 1)), mode
    # adversarial geometry with MASK / BLEND soups, the RT-pipeline flavour, sun & sky instead of the environment map
    ss = hd.default_sun_and_sky(); ss.in_use = 1
    cfg = Config(synth.fuzz_scene(2), env, 96, 64, depth=5, variant=capi.PT_VARIANT_RTX, sunsky=ss)
    assert _bits_equal(host_render(cfg, 3, two), render_oracle(cfg, 3)), "fuzz scene, RTX variant, sun & sky"
    # an image that is not a multiple of the tile size, depth of field
    sc = synth.fuzz_scene(4); sc.camera.aperture = 0.05
    cfg = Config(sc, env, 50, 37, depth=4, hdr_multiplier=2.0)
    assert _bits_equal(host_render(cfg, 2, two), render_oracle(cfg, 2)), "odd size, depth of field"


def test_host_build_renders_the_c3_stand_in_like_the_oracle():
    """the bench scene (269 k triangles, alpha-tested foliage cards with opacity maps, HDR environment, Disney BSDF, depth 8) at a reduced
    resolution, four frames: host build of the product's source == oracle, bit for bit, on both acceleration structures"""
    from tests.common import Config, render_oracle
    from vk_raytrace_amd import workloads
    wl = workloads.c3_sponza(160, 90, 4, tex_size=64, env_w=256)
    cfg = Config(wl.scene, wl.env, wl.width, wl.height, depth=wl.depth, pbr=wl.pbr_mode)
    ref = render_oracle(cfg, 4)
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0
    for two in (0, 1):
        assert _bits_equal(host_render(cfg, 4, two), ref), two


# ---- deep structures: the premise of tests/test_gpu_edges.py ----------------------------------------------------------------------------------
@pytest.mark.parametrize("two,merge", [(0, True), (1, True), (1, False)])
def test_deep_chain_reaches_the_spill_array_and_the_overflow(two, merge):
    """synth.deep_chain at DEEP_SPILL_LEVELS: camera, bounce and shadow walks of the default builder's structure (device binned SAH, host
    emulation) reach stack levels 25..64 -- beyond the LDS part (STACK_LDS = 24 entries), within the private spill array -- and none overflows.
    At DEEP_OVERFLOW_LEVELS walks need more than 64 entries.  If a builder change flattens these trees this test fails, instead of the GPU
    tests passing without reaching the spill path."""
    from tests.common import Config
    rng = np.random.default_rng(17)
    env = synth.procedural_sky(64, 32)
    tr = TracedScene(synth.deep_chain(synth.DEEP_SPILL_LEVELS), merge_singles=merge)
    deep = TracedScene(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), merge_singles=merge)
    cfg = Config(synth.deep_chain(synth.DEEP_SPILL_LEVELS), env, 64, 48)
    o, d = deep_rays(cfg)
    seeds = np.arange(len(o), dtype=np.uint32)
    w, tuv, _, _, hist, over = tr.settle(0, two, 2, o, d, seeds, sp_hist=True)
    assert over == 0
    assert hist[64] == 0 and hist[25:64].sum() > 0.4 * hist.sum(), hist       # camera rays: most walks spill
    hit = w != NONE
    assert hit.mean() > 0.5
    # bounce rays from where they hit, transmitted onwards (+z: the thin-walled slivers' main lobe), and shadow rays along the same
    # directions (towards the environment's +z hemisphere, unbounded and bounded)
    p = (o + d * tuv[:, :1])[hit]
    k = len(p)
    b = rng.normal(0, 1, (k, 3)); b[:, 2] = np.abs(b[:, 2]) + 1.0
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    start = p + b * (1e-4 * np.abs(p).max(1, keepdims=True))
    for kind, tmax in ((0, None), (1, np.full(k, 1e30, np.float32)), (1, rng.uniform(1e5, 1e7, k).astype(np.float32))):
        _, _, _, _, hist, over = tr.settle(kind, two, 2, start, b, seeds[:k], tmax, sp_hist=True)
        assert over == 0, kind
        assert hist[64] == 0 and hist[25:64].sum() > 0.02 * hist.sum(), (kind, hist)   # bounce and shadow walks spill too
    _, _, _, _, hist, over = deep.settle(0, two, 2, o, d, seeds, sp_hist=True)
    assert over > 0 and hist[64] > 0.1 * hist.sum(), (over, hist)         # a share of the camera walks needs more than 64 entries
    tr.close(); deep.close()


def test_host_build_renders_the_spill_scene_like_the_oracle():
    """the same deep scene through the product's shading source on the host (lock-step walks of k_tail, spill array included) == oracle"""
    from tests.common import Config, render_oracle
    cfg = Config(synth.deep_chain(synth.DEEP_SPILL_LEVELS), synth.procedural_sky(128, 64), 48, 32, depth=5, max_samples=2)
    ref = render_oracle(cfg, 2)
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0
    for two in (0, 1):
        assert _bits_equal(host_render(cfg, 2, two), ref), two


# ---- the harness's own build ------------------------------------------------------------------------------------------------------------------------
def test_the_recorded_dependencies_name_every_file_the_build_reads():
    """the library is rebuilt when a file of this list is newer than it: the list must hold the headers of the public interface and of the
    transcendental contract, the product's internal header, and every unit and header of the harness"""
    import glob
    import os
    deps = set(host_harness.deps())
    assert {"include/pt_fpmath.h", "include/pt_types.h", "vk_raytrace_amd/csrc/pt_internal.h"} <= deps
    for h in ("pt_trace.h", "pt_machine.h", "pt_settle.h", "pt_shade.h", "pt_probe.h", "pt_query.h"):
        assert "vk_raytrace_amd/csrc/" + h in deps, h
    units = {"tests/cpp/" + u for u in host_harness.UNITS} | {os.path.relpath(h, host_harness.ROOT) for h in glob.glob(os.path.join(host_harness.CPP, "*.h"))}
    assert {"tests/cpp/trace_host.cpp", "tests/cpp/th_shims.h", "tests/cpp/th_scene.h", "tests/cpp/th_walk.h"} <= units
    assert units <= deps, sorted(units - deps)


def test_the_signature_table_and_the_library_name_the_same_entry_points():
    """every entry of the table resolves in the default library (lib() fails otherwise), and the library exports no th_* / qh_* symbol the table
    does not declare -- such a symbol would be called with ctypes' defaults, a pointer passed as a C int"""
    if shutil.which("nm") is None:
        pytest.skip("nm is not installed")
    L = host_harness.lib()
    table = [name for name, _, _ in host_harness.SIGNATURES]
    assert len(set(table)) == len(table)
    for name in table:
        assert getattr(L, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", host_harness.build()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith(("th_", "qh_"))}
    assert exported == set(table), (sorted(exported - set(table)), sorted(set(table) - exported))
    experiments = {name for sigs in host_harness.EXPERIMENT_SIGNATURES.values() for name, _, _ in sigs}
    assert not experiments & exported, "experiment entry points stay out of the default library"

"""The device-built acceleration structures read back and audited node by node (tests/accel_audit.py; proved on planted defects by
tests/test_accel_audit.py).  Every case is a build the product runs anyway and one copy of its arrays: no frame is rendered, no kernel is added.
Flat structure: every scene under every builder.  Two-level structure: the forest scene under every builder, with and without the merged world-space
structure and the build arena; the remaining settings pairwise.  State changes on one context; tree quality against the builder's emulation."""
import contextlib
import json
import os

import numpy as np
import pytest

from tests import accel_audit as A
from vk_raytrace_amd import capi

pytestmark = pytest.mark.gpu
BUILDERS = ["sahdev", "sah", "ploc", "lbvh"]
TOL_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accel_audit_tol.json")

SCENES = {f"soup{n}": (lambda n=n: A.soup(n)) for n in A.LADDER}
SCENES.update(coincident=A.coincident, zero_area=A.zero_area, half_coincident=A.half_coincident, forest=A.forest)
GROUPS = {   # a few builds per test id
    "tiny": [f"soup{n}" for n in (1, 2, 3, 4, 5, 12, 13, 14)],
    "wave_block": [f"soup{n}" for n in (63, 64, 65, 255, 256, 257)],
    "degenerate": ["coincident", "zero_area", "half_coincident", "forest"],
    "sort_edge": [f"soup{n}" for n in (2047, 2048, 2049, 5000)],
}
_scene_cache = {}


def scene(name):
    if name not in _scene_cache:
        sc = SCENES[name]()
        sc.finalize(capi.pack_vertices)
        _scene_cache[name] = sc
    return _scene_cache[name]


@contextlib.contextmanager
def context(tune):
    """a context created under PT_TUNE=tune (pt_create reads the variable); the environment is put back"""
    from vk_raytrace_amd.renderer import HipRenderer
    old = os.environ.get("PT_TUNE")
    os.environ["PT_TUNE"] = tune
    r = HipRenderer()
    try:
        r.setup(0)
        yield r
    finally:
        r.destroy()
        if old is None:
            os.environ.pop("PT_TUNE", None)
        else:
            os.environ["PT_TUNE"] = old


def build_and_audit(r, sc, what, merge=True, any_hit=True):
    r.set_scene(sc)
    d = A.device_dump(r)
    rep = A.audit(d, A.scene_inputs(sc, any_hit=any_hit, merge_singles=merge))
    A.assert_clean(rep, what)
    return d, rep


# ---- flat: scenes x builders ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("builder", BUILDERS)
def test_flat_structure(builder, group):
    forms = set()
    with context(f"build={builder},cnodes=1") as r:
        for name in GROUPS[group]:
            d, rep = build_and_audit(r, scene(name), f"flat {builder} {name}")
            i = d["info"]
            assert i["accelMode"] == 0 and i["numTris"] == scene(name).num_triangles and i["haveCNodes"] == 1 and i["builder"] == {"lbvh": 0, "sah": 1, "ploc": 2, "sahdev": 3}[builder]
            assert d["BVH2"] is not None and (d["SHADE_TRIS"] is not None) == bool(i["haveShadeTris"])
            assert [n for n in rep["_facts"]["not_checked"] if n in ("WIDE", "CNODES", "TRIS", "ALPHA_RECS", "BVH2", "SHADE_TRIS")] == []
            forms.add(A.padding_form(rep))
    print(f"padding form, flat {builder} {group}: {sorted(forms)}")
    assert forms <= {"separate", "undecided"}, forms   # the library is compiled without contraction: DESIGN.md, tri_box contract


# ---- two-level: forest x builders x mergeSingles x arena -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", [1, 0])
@pytest.mark.parametrize("builder", BUILDERS)
def test_two_level_forest(builder, merge):
    for arena in (1, 0):
        with context(f"build={builder},accel=two,mergeSingles={merge},arena={arena},cnodes=1") as r:
            d, rep = build_and_audit(r, scene("forest"), f"two-level {builder} mergeSingles={merge} arena={arena}", merge=bool(merge))
            i = d["info"]
            assert i["accelMode"] == 1 and i["haveCNodes"] == 1 and (i["mergedTris"] > 0) == bool(merge)
            assert i["numBlas"] == len(d["BLAS_RANGES"]) + (1 if merge else 0)
            assert [n for n in rep["_facts"]["not_checked"] if n not in ("BVH2", "SHADE_TRIS") and not (n == "MERGED_LIST" and not merge)] == []


# ---- the remaining settings, pairwise ------------------------------------------------------------------------------------------------------------
PAIRWISE = [   # (PT_TUNE, mergeSingles, scenes): every value of blasWorkers, cnodes, arena and mergeSingles meets every builder and both small and large scenes
    ("build=sahdev,accel=two,mergeSingles=0,blasWorkers=1,cnodes=0", 0, ["soup1", "soup13", "soup257", "forest"]),
    ("build=sah,accel=two,mergeSingles=1,blasWorkers=1,cnodes=1,arena=0", 1, ["soup2", "soup64", "coincident", "forest"]),
    ("build=ploc,accel=two,mergeSingles=0,blasWorkers=1,cnodes=1,arena=0", 0, ["soup3", "soup2048", "zero_area", "forest"]),
    ("build=lbvh,accel=two,mergeSingles=1,blasWorkers=1,cnodes=0", 1, ["soup1", "soup14", "soup2049", "forest"]),
    ("build=sahdev,accel=two,mergeSingles=1,cnodes=0,arena=0", 1, ["soup1", "soup5", "soup5000"]),
    ("build=sah,accel=two,mergeSingles=0,cnodes=0", 0, ["soup4", "soup255", "half_coincident"]),
    ("build=ploc,accel=two,mergeSingles=1,cnodes=0", 1, ["soup12", "soup65", "soup2047"]),
    ("build=lbvh,accel=two,mergeSingles=0,cnodes=1,arena=0", 0, ["soup63", "soup256", "soup5000"]),
    ("build=sahdev,cnodes=0,arena=0", 1, ["soup1", "soup13", "soup2049", "forest"]),
    ("build=lbvh,cnodes=0,arena=0", 1, ["soup2", "soup64", "zero_area"]),
    ("build=ploc,cnodes=0,arena=0", 1, ["soup14", "soup257", "coincident"]),
    ("build=sah,cnodes=0,arena=0", 1, ["soup3", "soup2048", "half_coincident"]),
]


@pytest.mark.parametrize("tune,merge,names", PAIRWISE, ids=[p[0] for p in PAIRWISE])
def test_settings_pairwise(tune, merge, names):
    with context(tune) as r:
        for name in names:
            d, rep = build_and_audit(r, scene(name), f"{tune} {name}", merge=bool(merge))
            assert d["info"]["haveCNodes"] == (1 if "cnodes=1" in tune else 0)
            assert d["info"]["accelMode"] == (1 if "accel=two" in tune else 0)


# ---- state changes on one context ----------------------------------------------------------------------------------------------------------------
def _moved(sc, which, seed):
    """a copy of the scene's node list with the nodes `which` moved (rotated, rescaled, shifted)"""
    from vk_raytrace_amd.scene import translate, rotate_y, scale
    import copy
    rng = np.random.default_rng(seed)
    out = copy.copy(sc)
    out.nodes = list(sc.nodes)
    for i in which:
        m, pm = out.nodes[i]
        out.nodes[i] = ((translate(*rng.uniform(-2, 2, 3)) @ m @ rotate_y(rng.uniform(0, 6.3)) @ scale(*rng.uniform(0.7, 1.4, 3))).astype(np.float32), pm)
    return out


def _used_refs(W, rows):
    c = W[rows, 24:28]
    return c[c != A.BVH_NONE]


def test_two_level_state_changes():
    sc = scene("forest")
    with context("accel=two,mergeSingles=1,cnodes=1") as r:
        d0, _ = build_and_audit(r, sc, "forest, built")
        S0 = A.scene_inputs(sc)
        merged = set(d0["MERGED_LIST"].tolist())
        active = [i for i in range(len(S0["inst"])) if S0["inst"]["triCount"][i] and i not in merged]
        assert len(merged) >= 2 and len(active) >= 4 and d0["info"]["mergedWide"] > 0
        # 1. only instances with an object-space BLAS move: a TLAS refit, everything below it stays
        sc1 = _moved(sc, active[::2], 1)
        r.update_instances(sc1)
        d1 = A.device_dump(r)
        A.assert_clean(A.audit(d1, A.scene_inputs(sc1)), "after an update of non-merged instances")
        for name in ("WIDE", "TRIS", "ALPHA_RECS", "CNODES"):
            assert np.array_equal(d0[name], d1[name]), name
        assert not np.array_equal(d0["TLAS"], d1["TLAS"])
        # 2. a merged instance moves: the merged structure is rebuilt in place, the object-space BLASes stay
        sc2 = _moved(sc1, sorted(merged)[:1], 2)
        r.update_instances(sc2)
        d2 = A.device_dump(r)
        A.assert_clean(A.audit(d2, A.scene_inputs(sc2)), "after an update of a merged instance")
        assert np.array_equal(d1["BLAS_RANGES"], d2["BLAS_RANGES"])
        for base, num in d2["BLAS_RANGES"]:
            assert np.array_equal(d1["WIDE"][base:base + num], d2["WIDE"][base:base + num]), base
        assert not np.array_equal(d1["WIDE"][:d1["info"]["mergedWide"]], d2["WIDE"][:d1["info"]["mergedWide"]])
        # 3. useAnyHit(false): every triangle is opaque, no reference carries the tag
        r.useAnyHit(False)
        d3 = A.device_dump(r)
        A.assert_clean(A.audit(d3, A.scene_inputs(sc2, any_hit=False)), "after pt_use_any_hit(0)")
        rows = np.concatenate([np.arange(d3["info"]["mergedWide"])] + [np.arange(b, b + n) for b, n in d3["BLAS_RANGES"]])
        assert not (_used_refs(d3["WIDE"], rows) & A.BVH_ALPHA).any() and not (_used_refs(d3["TLAS"], np.arange(len(d3["TLAS"]))) & A.BVH_ALPHA).any()
        r.useAnyHit(True)
        d4 = A.device_dump(r)
        A.assert_clean(A.audit(d4, A.scene_inputs(sc2)), "after pt_use_any_hit(1)")
        assert (_used_refs(d4["WIDE"], rows) & A.BVH_ALPHA).any()   # the MASK mesh is back
        # 4. to the flat structure and back
        r.set_accel_mode(capi.PT_ACCEL_FLAT)
        df = A.device_dump(r)
        assert df["info"]["accelMode"] == 0 and df["TLAS"] is None
        A.assert_clean(A.audit(df, A.scene_inputs(sc2)), "flat after pt_set_accel_mode")
        r.set_accel_mode(capi.PT_ACCEL_TWO_LEVEL)
        A.assert_clean(A.audit(A.device_dump(r), A.scene_inputs(sc2)), "two-level after pt_set_accel_mode")


def test_flat_update_is_a_rebuild():
    sc = scene("forest")
    with context("cnodes=1") as r:
        build_and_audit(r, sc, "forest flat, built")
        sc1 = _moved(sc, range(0, len(sc.nodes), 3), 5)
        r.update_instances(sc1)
        A.assert_clean(A.audit(A.device_dump(r), A.scene_inputs(sc1)), "flat after pt_update_instances")


def test_read_back_refuses_a_short_buffer_and_a_missing_structure():
    import ctypes as C
    with context("") as r:
        L, ctx = r._lib, r._ctx
        buf = np.full(64, 0xABABABAB, np.uint32)
        assert L.pt_debug_accel_read(ctx, 0, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_STATE
        assert L.pt_debug_accel_info(ctx, buf.ctypes.data, 21) == capi.PT_ERR_STATE
        r.set_scene(scene("soup5"))
        have = L.pt_debug_accel_read(ctx, 2, None, 0)
        assert have == capi.PT_ERR_INVALID
        assert L.pt_debug_accel_read(ctx, 2, buf.ctypes.data, 5 * 48 - 4) == capi.PT_ERR_INVALID and (buf == 0xABABABAB).all()   # nothing copied
        assert L.pt_debug_accel_read(ctx, 2, buf.ctypes.data, buf.nbytes) == 5 * 48
        assert L.pt_debug_accel_read(ctx, 5, buf.ctypes.data, buf.nbytes) == 0     # no TLAS in flat mode
        assert L.pt_debug_accel_read(ctx, 99, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_INVALID


# ---- quality: the device's trees against the builder's emulation ---------------------------------------------------------------------------------
def cost_ratios(builder, name):
    """cost(device) / cost(harness) per hierarchy: the flat structure, and for the forest the hierarchies of the two-level structure.  The harness tree is
    the device binned-SAH builder's emulation without its rotation passes (tests/cpp/th_scene.h)"""
    from tests.host_harness import TracedScene
    sc = scene(name)
    tr = TracedScene(sc, merge_singles=True, compact_nodes=False)
    out = {}
    for two in ((0, 1) if name == "forest" else (0,)):
        ref = A.cost(A.harness_dump(tr, two))
        with context(f"build={builder}" + (",accel=two" if two else "")) as r:
            r.set_scene(sc)
            dev = A.cost(A.device_dump(r))
        assert set(dev) == set(ref), (sorted(dev), sorted(ref))
        for k in sorted(ref):
            out[k] = dev[k] / ref[k] if ref[k] > 0 else (1.0 if dev[k] == 0 else float("inf"))
    tr.close()
    return out


@pytest.mark.parametrize("name", ["soup5000", "forest"])
@pytest.mark.parametrize("builder", ["sahdev", "sah"])
def test_tree_quality_matches_the_emulation(builder, name):
    """The rotation passes the emulation leaves out can only lower the cost, and the emulation is pinned to the host SAH builder within 1e-3
    (tests/test_sah_cpu.py): device <= harness x (1 + m), m and the measured ratios in tests/golden/accel_audit_tol.json"""
    m = json.load(open(TOL_FILE))["m"]
    ratios = cost_ratios(builder, name)
    print(f"cost ratios {builder} {name}: " + ", ".join(f"{k} {v:.6f}" for k, v in ratios.items()))
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0 + m, (builder, name, worst, ratios[worst])

"""The refit of csrc/pt_refit.h on the CPU (tests/cpp/refit_host.cpp: the bodies the kernels of pt_refit.hip run, one arrival after the other) on the
structures of the host harness, flat and two-level, for the scenes of tests/accel_audit.py: the size ladder of soups, the degenerate soups and the
forest.  The refitted dump is judged by the auditor against the DEFORMED vertices; the topology, the costs, the unchanged-vertices identity, planted
defects, the harness's own walk on the refitted structure and a sanitizer run of the same unit as a stand-alone program follow."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import accel_audit as A
from tests import host_harness as H
from tests import refit_host as R

U, F = np.uint32, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {**{f"soup{n}": (lambda n=n: A.soup(n)) for n in A.LADDER}, "coincident": A.coincident, "zero_area": A.zero_area, "half_coincident": A.half_coincident, "forest": A.forest}
ARRAYS = ["WIDE", "TRIS", "ALPHA_RECS", "CNODES"]
_cache = {}


def case(name):
    """per scene, computed once and never modified: the inputs before and after the deformation, and per mode the harness dump, the refitted dump,
    the root boxes and the costs.  The instance hierarchy of the two-level dump is the harness's over the deformed scene: the product builds it again too"""
    if name not in _cache:
        scene = SCENES[name]()
        new, _ = R.deform(scene, seed=11)
        S0, S1 = A.scene_inputs(scene), A.scene_inputs(new)
        tr, tr1 = H.TracedScene(scene, merge_singles=True, compact_nodes=True), H.TracedScene(new, merge_singles=True, compact_nodes=True)
        modes = []
        for two in (0, 1):
            d0 = A.harness_dump(tr, two)
            d1, boxes, costs = R.refit_dump(d0, S0, S1)
            if two:
                fresh = A.harness_dump(tr1, 1)
                for k in ("TLAS", "CTLAS", "TLAS_LEAVES"):
                    d1[k] = fresh[k].copy()
                # (a leaf names its BLAS by node base, and the bases are those of the structure that was refitted)
                base_of = dict(zip(d0["TLAS_LEAVES"][:, 0].tolist(), d0["TLAS_LEAVES"][:, 1].tolist()))
                d1["TLAS_LEAVES"][:, 1] = [base_of[i] for i in d1["TLAS_LEAVES"][:, 0].tolist()]
                d1["info"]["numTlasNodes"] = fresh["info"]["numTlasNodes"]
            modes.append((d0, d1, boxes, costs))
        tr.close(); tr1.close()
        _cache[name] = (scene, new, S0, S1, modes)
    return _cache[name]


@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("name", list(SCENES))
def test_refitted_structure_is_clean_and_keeps_its_topology(name, two):
    scene, new, S0, S1, modes = case(name)
    d0, d1, boxes, costs = modes[two]
    A.assert_clean(A.audit(d0, S0), f"{name} two={two} as built")
    A.assert_clean(A.audit(d1, S1), f"{name} two={two} refitted")
    # every child word and every record's .w is what it was
    assert np.array_equal(d0["WIDE"][:, 24:28], d1["WIDE"][:, 24:28])
    assert np.array_equal(d0["TRIS"][:, [3, 7, 11]], d1["TRIS"][:, [3, 7, 11]]) and np.array_equal(d0["ALPHA_RECS"][:, 6:8], d1["ALPHA_RECS"][:, 6:8])
    assert np.array_equal(d0["CNODES"][:, 16:20], d1["CNODES"][:, 16:20])
    # ... and every box was made again: a refit that skipped nodes would not pass
    assert R.used_boxes_all_changed(d0, d1) >= len(d0["TRIS"])
    # the stale dump is NOT clean against the deformed vertices (the audit sees what the refit is for)
    assert {"tri_record", "leaf_box"} <= set(A.failing(A.audit(d0, S1)))
    # costs: N * 2^-53 relative for N < 1e6 non-negative double terms, times a generous constant
    for got, dump in ((costs[0], d0), (costs[1], d1)):
        want = sum(v for k, v in A.cost(dump).items() if k != "tlas")
        assert abs(got - want) <= 1e-9 * want, (got, want)
    # the root's union: the merged box in two-level mode (audited above as merged_box), the world bounds in flat mode
    if not two:
        lo, hi = A._boxes(d1["WIDE"][0:1])
        used = d1["WIDE"][0, 24:28] != A.BVH_NONE
        assert np.array_equal(boxes[0, 0:3], lo[0][used].min(0)) and np.array_equal(boxes[0, 3:6], hi[0][used].max(0))


@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("name", ["soup1", "soup2", "soup5", "soup257", "zero_area", "forest"])
def test_refit_with_unchanged_vertices_changes_no_word(name, two):
    scene, new, S0, S1, modes = case(name)
    d0 = modes[two][0]
    same, boxes, costs = R.refit_dump(d0, S0, S0)
    for k in ARRAYS:
        a, b = same[k].copy(), d0[k].copy()
        if k == "WIDE":   # the harness's collapse writes no order table (a zero pad decodes to slot order); the device's does: tests/test_refit_gpu.py holds those bytes
            assert not b[:, 28:32].any()
            a[:, 28:30] = 0
        assert np.array_equal(a, b), k
    assert abs(costs[0] - costs[1]) <= 1e-12 * costs[0]   # (the same terms, added in another order)
    d1 = modes[two][1]
    again, _, c2 = R.refit_dump(d1, S0, S1)   # a second refit over the refitted arrays: every word, the order bytes in WideNode::pad included
    for k in ARRAYS:
        assert np.array_equal(again[k], d1[k]), k
    # the order bytes are those of pt_order.h for the refitted planes: the packet-order test's encoder is the kernel's, so decode and check they are a permutation
    pad = d1["WIDE"][:, 28:30]
    ranges, _ = R.tables(d0, S0)
    for base, num in ranges:
        by = (pad[base:base + num, :, None] >> (8 * np.arange(4, dtype=U))) & 0xFF ^ 0xE4
        perm = np.stack([(by >> (2 * j)) & 3 for j in range(4)], -1)
        assert (np.sort(perm, -1) == np.arange(4)).all()


@pytest.mark.parametrize("two", [0, 1])
def test_planted_defects_are_reported(two):
    scene, new, S0, S1, modes = case("forest")
    d0, d1, _, _ = modes[two]
    copy = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d1.items()}
    # one node's union skipped: an inner reference keeps the box it had before the refit
    W = d1["WIDE"]
    ch = W[:, 24:28]
    inner = (ch != A.BVH_NONE) & ((ch & A.BVH_LEAF) == 0)
    node, k = [int(x[len(x) // 2]) for x in np.nonzero(inner)]
    bad = copy()
    bad["WIDE"][node, k:24:4] = d0["WIDE"][node, k:24:4]
    assert "inner_box" in A.failing(A.audit(bad, S1))
    # one leaf record left stale
    bad = copy()
    s = len(d1["TRIS"]) // 2
    bad["TRIS"][s] = d0["TRIS"][s]
    got = A.failing(A.audit(bad, S1))   # (a BLAS whose records are not its mesh's is also reported as naming no mesh)
    assert "tri_record" in got and set(got) <= {"tri_record", "tlas_leaf_node_base"}
    # compact nodes not made again
    bad = copy()
    bad["CNODES"] = d0["CNODES"].copy()
    assert any(c.startswith("cnode_") for c in A.failing(A.audit(bad, S1)))


@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("name", ["soup257", "forest"])
def test_harness_walk_on_the_refitted_structure_equals_brute_force(name, two):
    """flat: the refitted arrays go back into the scene they were dumped from, with the deformed vertices.  Two-level: the refitted merged structure and
    BLASes (world-form and vertex-form records, their boxes, the compact nodes) go under the instance hierarchy of the harness's build of the deformed
    scene, whose leaves then name the refitted structure's node bases -- what pt_refit_accel leaves -- and the two-level walk runs through the padded
    instance boxes into them"""
    scene, new, S0, S1, modes = case(name)
    d0, d1, _, _ = modes[two]
    tr = H.TracedScene(new if two else scene, merge_singles=True, compact_nodes=True)
    try:
        L = R.scene_lib()
        if two:
            base = np.ascontiguousarray(d0["INST_NODE_BASE"], U)
            rc = L.rfh_scene_set_two(tr.h, len(d1["WIDE"]), d1["WIDE"].ctypes.data, len(d1["TRIS"]), d1["TRIS"].ctypes.data, d1["ALPHA_RECS"].ctypes.data, d1["CNODES"].ctypes.data,
                                     len(base), base.ctypes.data)
            after = A.harness_dump(tr, 1)   # the scene now holds the refitted arrays: what the walk below reads is what the auditor accepts
            for k in ("WIDE", "TRIS", "ALPHA_RECS", "CNODES", "TLAS_LEAVES"):
                assert np.array_equal(after[k], d1[k]), k
        else:
            v = np.ascontiguousarray(S1["vertices"], F)
            rc = L.rfh_scene_set_flat(tr.h, len(v), v.ctypes.data, len(d1["WIDE"]), d1["WIDE"].ctypes.data, len(d1["TRIS"]), d1["TRIS"].ctypes.data, d1["ALPHA_RECS"].ctypes.data,
                                      d1["CNODES"].ctypes.data)
        assert rc == 0
        org, dirs = H.rays_for(tr, np.random.default_rng(5), np.zeros(3), 400)
        ref_w, ref_t = tr.candidates(0, org, dirs, max_cand=2)   # brute force over the deformed world triangles
        w, t = tr.candidates(1 + two, org, dirs, max_cand=2)
        assert (ref_w[:, 0] != H.NONE).sum() > 150
        H.accidental_differences(tr, org, dirs, ref_w, ref_t, w, t, f"{name}: {'two-level' if two else 'flat'} walk on the refitted structure")
        # the deformation moved the hits: the structure as built does not describe these triangles
        assert not np.array_equal(S0["vertices"], S1["vertices"]) and not np.array_equal(d0["TRIS"], d1["TRIS"])
    finally:
        tr.close()


def _write_case(path, dump, S_built, S_new):
    ranges, slots = R.tables(dump, S_built)
    cn = dump.get("CNODES") if dump["info"]["haveCNodes"] else None
    nshade = dump["info"]["numTris"] if dump["info"]["accelMode"] == 0 else 0
    inst = np.ascontiguousarray(S_new["inst"])
    head = np.array([len(dump["WIDE"]), len(dump["TRIS"]), len(ranges), len(slots), len(inst), len(S_new["vertices"]), len(S_new["indices"]), 0 if cn is None else 1, nshade], U)
    with open(path, "wb") as f:
        for a in (head, dump["WIDE"], dump["TRIS"], dump["ALPHA_RECS"], ranges, slots, inst.view(U), np.ascontiguousarray(S_new["vertices"], F).view(U), S_new["indices"]) + \
                 ((cn,) if cn is not None else ()) + (np.zeros((nshade, 32), U),):
            f.write(np.ascontiguousarray(a).tobytes())


def test_refit_unit_runs_clean_under_the_sanitizers():
    """tests/cpp/refit_asan_main.cpp: the same unit as a stand-alone program built with -fsanitize=address,undefined, every array in a heap block of its own size"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "refit_asan")
        subprocess.check_call(["g++"] + [c for c in H.COMPILE if c not in ("-fopenmp", "-fPIC")] + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                                                                                                  os.path.join(ROOT, "tests", "cpp", "refit_asan_main.cpp")])
        files = []
        for name in ("soup257", "forest"):
            scene, new, S0, S1, modes = case(name)
            for two in (0, 1):
                files.append(os.path.join(tmp, f"{name}_{two}.bin"))
                _write_case(files[-1], modes[two][0], S0, S1)
        p = subprocess.run([exe] + files, capture_output=True, text=True)
        assert p.returncode == 0 and "refit cases 4" in p.stdout, (p.stdout + p.stderr)[-800:]

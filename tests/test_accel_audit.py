"""The auditor of the built acceleration structures (tests/accel_audit.py) proved on the CPU: it accepts the structures the host harness assembles
(tests/cpp/th_scene.h: the device builder's emulation + the restated stages) on the scenes the trace tests walk and on the size ladder the device
tests build, and it reports every planted defect under the defect's own check.  A check of the auditor without a planted defect fails the file."""
import copy

import numpy as np
import pytest

from tests import accel_audit as A
from tests.host_harness import TracedScene, instanced_scene

U, F = np.uint32, np.float32


def _audit_harness(scene, merge, compact):
    tr = TracedScene(scene, merge_singles=merge, compact_nodes=compact)
    S = A.scene_inputs(scene, merge_singles=merge)
    out = []
    for two in (0, 1):
        d = A.harness_dump(tr, two)
        assert bool(d["info"]["haveCNodes"]) == bool(compact)
        out.append((d, A.audit(d, S)))
    tr.close()
    return S, out


# ---- accepts a good structure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge,compact", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("name", ["instanced3", "instanced11far", "fuzz0", "fuzz5", "forest"])
def test_harness_structures_are_clean(name, merge, compact):
    from vk_raytrace_amd import synth
    scene = {"fuzz0": lambda: synth.fuzz_scene(0), "fuzz5": lambda: synth.fuzz_scene(5), "instanced3": lambda: instanced_scene(3)[0], "instanced11far": lambda: instanced_scene(11, n_nodes=90, far=True)[0], "forest": A.forest}[name]()
    _, out = _audit_harness(scene, merge, compact)
    for two, (d, rep) in enumerate(out):
        A.assert_clean(rep, f"{name} merge={merge} compact={compact} two={two}")
        # what the harness cannot supply is reported as not checked, nothing else
        absent = {"BVH2", "INST_PAD", "ACTIVE", "SHADE_TRIS"} | (set() if compact else {"CNODES", "CTLAS"})
        if two:
            assert set(rep["_facts"]["not_checked"]) - {"MERGED_LIST", "BLAS_RANGES"} == absent
        assert A.padding_form(rep) in ("separate", "undecided")   # the harness is compiled without contraction


@pytest.mark.parametrize("n", A.LADDER)
def test_harness_ladder_is_clean(n):
    _, out = _audit_harness(A.soup(n), True, True)
    for two, (d, rep) in enumerate(out):
        A.assert_clean(rep, f"soup{n} two={two}")
    assert out[0][0]["info"]["numTris"] == n


@pytest.mark.parametrize("make", [A.coincident, A.zero_area, A.half_coincident], ids=lambda f: f.__name__)
def test_harness_degenerate_soups_are_clean(make):
    _, out = _audit_harness(make(), True, True)
    for two, (d, rep) in enumerate(out):
        A.assert_clean(rep, f"{make.__name__} two={two}")
    if make is A.zero_area:   # boxes that start at 0 and end at 1e-25 show the padding's two roundings
        assert A.padding_form(out[0][1]) == "separate"


# ---- rejects planted defects ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean():
    """clean dumps of the forest scene (merged structure, 7 BLASes, TLAS, compact nodes) -- never modified: every mutation works on a copy"""
    scene = A.forest()
    S, out = _audit_harness(scene, True, True)
    flat, two = out[0][0], out[1][0]
    # the two arrays of the flat structure the harness does not keep, in the form pt_device.h gives them: the binary root (both child boxes = the
    # root's box) and the shading lines' identity quad
    lo, hi = A._boxes(flat["WIDE"][0:1])
    used = flat["WIDE"][0, 24:28] != A.BVH_NONE
    rlo, rhi = lo[0][used].min(0), hi[0][used].max(0)
    b = np.zeros((1, 16), U)
    b[0, 0:12] = A._u(np.concatenate([rlo, rhi, rlo, rhi]))
    b[0, 12:14] = (1, 2)
    flat["BVH2"] = b
    sh = np.zeros((len(flat["TRIS"]), 32), U)
    sh[:, 24], sh[:, 25] = flat["TRIS"][:, 7], flat["TRIS"][:, 11]
    flat["SHADE_TRIS"] = sh
    # ... and the two input lists of the TLAS build, as pt_capi_accel.hip's comments give them: the active instances, the padding constants per instance
    merged = set(two["MERGED_LIST"].tolist())
    act = np.array([i for i in range(len(S["inst"])) if S["inst"]["triCount"][i] and i not in merged], U)
    two["ACTIVE"] = act
    two["INST_PAD"] = np.zeros((len(S["inst"]), 2), U)
    two["INST_PAD"][act] = A._u(S["pad"][act])
    for d in (flat, two):
        A.assert_clean(A.audit(d, S))
    return S, flat, two


def _next(bits, up):
    """float32 bit pattern one ulp up / down"""
    f = np.array([bits], U).view(F)
    return np.nextafter(f, F(np.inf) if up else F(-np.inf)).view(U)[0]


def _levels(W, root=0):
    h = A._Hier(0, W, root, None, 0, 0, 0)
    levels, leaves, _ = A._walk(h, A._Report())
    return levels, leaves


def _find_ref(W, root, want_leaf, pred=lambda n, k: True):
    levels, _ = _levels(W, root)
    for lv in levels:
        for n in lv:
            for k in range(4):
                c = W[n, 24 + k]
                if c != A.BVH_NONE and bool(c & A.BVH_LEAF) == want_leaf and pred(int(n), k):
                    return int(n), k
    raise AssertionError("no such reference")


def _subtree_has_alpha(W, node):
    _, leaves = _levels(W, node)
    return bool((leaves[:, 2] & A.BVH_ALPHA).any())


def _blas(two, tris):
    """(range index, base) of a BLAS with that many triangles"""
    for k, (base, num) in enumerate(two["BLAS_RANGES"]):
        h = A._Hier(0, two["WIDE"], int(base), None, 0, 0, 0)
        if A._blas_slots(h)[1] == tris:
            yield k, int(base)


def m_inner_box_in(S, flat, two):
    n, k = _find_ref(two["WIDE"], 0, False)
    two["WIDE"][n, 0 + k] = _next(two["WIDE"][n, 0 + k], True)   # minx of child k: one ulp inwards


def m_inner_box_out(S, flat, two):
    n, k = _find_ref(two["WIDE"], 0, False)
    two["WIDE"][n, 0 + k] = _next(two["WIDE"][n, 0 + k], False)


def m_leaf_box_in(S, flat, two):
    n, k = _find_ref(two["WIDE"], 0, True)
    for _ in range(2):   # a leaf plane may lie within one ulp of either form of the padding (tests/accel_audit.py padded_box): the second ulp is the first one outside
        two["WIDE"][n, 4 + k] = _next(two["WIDE"][n, 4 + k], True)


def m_leaf_box_out(S, flat, two):
    n, k = _find_ref(two["WIDE"], 0, True)
    for _ in range(2):
        two["WIDE"][n, 4 + k] = _next(two["WIDE"][n, 4 + k], False)


def m_leaf_duplicated(S, flat, two):
    _, leaves = _levels(flat["WIDE"])
    (n0, k0, r0), (n1, k1, r1) = leaves[0], leaves[-1]
    flat["WIDE"][n1, 24 + k1] = r0


def m_ref_redirected(S, flat, two):
    W = flat["WIDE"]
    levels, _ = _levels(W)
    for n in levels[0]:
        inner = [k for k in range(4) if W[n, 24 + k] != A.BVH_NONE and not W[n, 24 + k] & A.BVH_LEAF]
        if len(inner) >= 2:
            W[n, 24 + inner[0]] = W[n, 24 + inner[1]]   # two references into one sibling's subtree, the other subtree lost
            return
    raise AssertionError("no node with two inner children")


def m_alpha_cleared(S, flat, two):
    W = flat["WIDE"]
    n, k = _find_ref(W, 0, False, lambda n, k: bool(W[n, 24 + k] & A.BVH_ALPHA))
    W[n, 24 + k] &= ~U(A.BVH_ALPHA)


def m_alpha_set(S, flat, two):
    W = flat["WIDE"]
    n, k = _find_ref(W, 0, False, lambda n, k: not W[n, 24 + k] & A.BVH_ALPHA)
    W[n, 24 + k] |= U(A.BVH_ALPHA)


def m_used_after_none(S, flat, two):
    W = flat["WIDE"]
    levels, _ = _levels(W)
    n = next(int(n) for lv in levels for n in lv if (W[n, 24:28] != A.BVH_NONE).sum() == 3)
    W[n, 3:24:4], W[n, 2:24:4] = W[n, 2:24:4].copy(), W[n, 3:24:4].copy()   # boxes of slots 2 and 3
    W[n, 27], W[n, 26] = W[n, 26], W[n, 27]


def m_tri_vertex(S, flat, two):
    flat["TRIS"][17, 5] = _next(flat["TRIS"][17, 5], True)


def m_world_index_swapped(S, flat, two):
    T = flat["TRIS"]
    T[3, 3], T[40, 3] = T[40, 3], T[3, 3]


def m_alpha_rec_swapped(S, flat, two):
    a = flat["ALPHA_RECS"]
    a[[5, 90]] = a[[90, 5]]


def m_cnode_plane_lowered(S, flat, two):
    c = flat["CNODES"][0]
    hi0 = (c[4 + 2] & 0xFFFF).astype(np.uint16)   # x axis, upper plane of child 0
    q = int(np.array([hi0], np.uint16).view(np.float16)[0])
    assert q >= 1
    c[4 + 2] = (c[4 + 2] & 0xFFFF0000) | int(np.array([q - 1], np.float16).view(np.uint16)[0])


def _half(q):
    return int(np.array([q], np.float16).view(np.uint16)[0])


def _plane(c, axis, child, upper):
    """(word, shift) of a plane of a compact node, and its value"""
    w, sh = 4 + 4 * axis + (2 if upper else 0) + child // 2, 16 * (child % 2)
    return w, sh, int(np.array([(c[w] >> sh) & 0xFFFF], np.uint16).view(np.float16)[0])


def m_cnode_lower_plane_loose(S, flat, two):
    C, W = flat["CNODES"], flat["WIDE"]
    for n in range(len(C)):
        for k in range(4):
            w, sh, q = _plane(C[n], 1, k, False)
            if W[n, 24 + k] != A.BVH_NONE and q >= 1:
                C[n, w] = (C[n, w] & ~U(0xFFFF << sh)) | U(_half(q - 1) << sh)
                return
    raise AssertionError("no lower plane above 0")


def m_cnode_origin(S, flat, two):
    flat["CNODES"][3, 0] = _next(flat["CNODES"][3, 0], False)


def m_cnode_empty_slot(S, flat, two):
    C, W = flat["CNODES"], flat["WIDE"]
    n = next(n for n in range(len(C)) if W[n, 27] == A.BVH_NONE)
    w, sh, q = _plane(C[n], 2, 3, True)
    C[n, w] |= U(_half(1) << sh)


def m_cnode_exponent(S, flat, two):
    flat["CNODES"][1, 3] += 1 << 8


def m_cnode_child(S, flat, two):
    two["CNODES"][2, 16] ^= 1


def m_cnode_uninitialised(S, flat, two):
    base = int(two["BLAS_RANGES"][-1, 0])
    two["CNODES"][base].view(np.uint8)[:] = 0xCD


def m_ctlas_uninitialised(S, flat, two):
    two["CTLAS"][0].view(np.uint8)[:] = 0xCD


def m_tlas_node_base(S, flat, two):
    (ka, a), (kb, b) = list(_blas(two, 64))[:2]
    L = two["TLAS_LEAVES"]
    s = np.nonzero(L[:, 1] == a)[0][0]
    L[s, 1] = b


def m_tlas_node_base_identical_mesh(S, flat, two):
    """the two 13-triangle meshes are the same geometry: only the one-BLAS-per-mesh rule and INST_NODE_BASE can tell"""
    (ka, a), (kb, b) = list(_blas(two, 13))[:2]
    L = two["TLAS_LEAVES"]
    s = np.nonzero(L[:, 1] == a)[0][0]
    L[s, 1] = b
    two["INST_NODE_BASE"] = None   # ... and here the table is not there to help


def m_pad_c1(S, flat, two):
    L = two["TLAS_LEAVES"]
    s = np.nonzero(L[:, 0] != A.PT_INST_MERGED)[0][0]
    L[s, 5] = _next(L[s, 5], True)


def m_instance_missing(S, flat, two):
    """one instance's leaf names another instance of the same mesh: the hierarchy is intact, an active instance is gone"""
    L, I = two["TLAS_LEAVES"], S["inst"]
    for s in np.nonzero(L[:, 0] != A.PT_INST_MERGED)[0]:
        twins = [j for j in np.nonzero(I["primMesh"] == I["primMesh"][L[s, 0]])[0] if j != L[s, 0]]
        if twins:
            L[s, 0] = twins[0]
            return
    raise AssertionError("no instanced mesh")


def m_inst_block(S, flat, two):
    two["INST_BLOCK"][1] += 1


def m_inst_tri_base(S, flat, two):
    two["INST_TRI_BASE"][4] += 1


def m_blas_range_overlap(S, flat, two):
    two["BLAS_RANGES"][2, 1] += 1


def m_merged_box(S, flat, two):
    two["info"]["mergedBox"] = two["info"]["mergedBox"].copy()
    two["info"]["mergedBox"][4] = np.nextafter(two["info"]["mergedBox"][4], F(np.inf))


def m_merged_list(S, flat, two):
    two["MERGED_LIST"] = two["MERGED_LIST"][:-1].copy()


def m_tlas_leaf_field(S, flat, two):
    L = two["TLAS_LEAVES"]
    s = np.nonzero(L[:, 0] != A.PT_INST_MERGED)[0][0]
    L[s, 2] ^= 1 << 29


def m_leaf_alpha_tag(S, flat, two):
    W = flat["WIDE"]
    n, k = _find_ref(W, 0, True, lambda n, k: bool(W[n, 24 + k] & A.BVH_ALPHA))
    W[n, 24 + k] &= ~U(A.BVH_ALPHA)


def m_empty_slot_box(S, flat, two):
    W = flat["WIDE"]
    levels, _ = _levels(W)
    n = next(int(n) for lv in levels for n in lv if W[n, 27] == A.BVH_NONE)
    W[n, 3] = 0   # minx of the empty slot


def m_ref_out_of_range(S, flat, two):
    W = two["TLAS"]
    n, k = _find_ref(W, 0, False)
    W[n, 24 + k] = (W[n, 24 + k] & ~U(A.BVH_SLOT_MASK)) | U(len(W) + 3)


def m_single_child(S, flat, two):
    """an inner node with one child (its box and tag are right: only the arity is wrong)"""
    W = flat["WIDE"]
    levels, _ = _levels(W)
    for lv in levels:
        for n in lv:
            if (W[n, 24:28] != A.BVH_NONE).sum() == 2 and (W[n, 24:26] & A.BVH_LEAF).all():
                W[n, 25] = A.BVH_NONE
                W[n, 1:12:4], W[n, 13:24:4] = A.FLT_MAX_BITS, A.NEG_FLT_MAX_BITS
                return
    raise AssertionError("no node with two leaves")


def m_stale_node_count(S, flat, two):
    two["info"]["numTlasNodes"] += 1


def m_active_list(S, flat, two):
    two["ACTIVE"][[1, 2]] = two["ACTIVE"][[2, 1]]


def m_active_count(S, flat, two):
    two["info"]["numActive"] -= 1


def m_inst_pad(S, flat, two):
    a = two["ACTIVE"][3]
    two["INST_PAD"][a, 0] = _next(two["INST_PAD"][a, 0], False)


def m_bvh2_root(S, flat, two):
    flat["BVH2"][0, 0] = _next(flat["BVH2"][0, 0], False)


def m_shade_tris(S, flat, two):
    flat["SHADE_TRIS"][9, 25] += 1


CN = {"cnode_child", "cnode_origin", "cnode_exponent", "cnode_plane", "cnode_enclose", "cnode_tight", "cnode_empty"}
# mutation -> (the checks that must report it, further checks that cover the mutated element and may report it too)
MUTATIONS = {
    m_inner_box_in: ({"inner_box"}, CN), m_inner_box_out: ({"inner_box"}, CN),
    m_leaf_box_in: ({"leaf_box"}, CN | {"inner_box", "merged_box"}), m_leaf_box_out: ({"leaf_box"}, CN | {"inner_box", "merged_box"}),
    m_leaf_duplicated: ({"leaf_permutation"}, {"cnode_child", "leaf_box", "leaf_alpha_tag", "inner_box", "inner_alpha_tag"}),
    m_ref_redirected: ({"node_reach"}, {"node_count", "leaf_permutation", "inner_box", "inner_alpha_tag", "cnode_child"}),
    m_alpha_cleared: ({"inner_alpha_tag"}, {"cnode_child"}), m_alpha_set: ({"inner_alpha_tag"}, {"cnode_child"}),
    m_used_after_none: ({"slot_order"}, CN),
    m_tri_vertex: ({"tri_record"}, set()), m_world_index_swapped: ({"tri_world_index"}, set()), m_alpha_rec_swapped: ({"alpha_rec"}, set()),
    m_cnode_plane_lowered: ({"cnode_enclose"}, set()), m_cnode_exponent: ({"cnode_exponent"}, {"cnode_tight", "cnode_enclose"}), m_cnode_child: ({"cnode_child"}, set()),
    m_cnode_lower_plane_loose: ({"cnode_tight"}, set()), m_cnode_origin: ({"cnode_origin"}, CN), m_cnode_empty_slot: ({"cnode_empty"}, set()),
    m_cnode_uninitialised: ({"cnode_child", "cnode_plane"}, CN), m_ctlas_uninitialised: ({"cnode_child", "cnode_plane"}, CN),
    m_tlas_node_base: ({"tlas_leaf_node_base"}, set()), m_tlas_node_base_identical_mesh: ({"tlas_leaf_node_base"}, set()),
    m_pad_c1: ({"tlas_leaf_pad"}, set()), m_instance_missing: ({"tlas_leaf_set"}, {"tlas_leaf_fields", "tlas_leaf_pad", "leaf_box", "leaf_alpha_tag"}),
    m_inst_block: ({"inst_block"}, set()), m_inst_tri_base: ({"inst_tri_base"}, set()), m_blas_range_overlap: ({"blas_ranges"}, {"node_reach", "node_count"}),
    m_merged_box: ({"merged_box"}, {"leaf_box"}), m_merged_list: ({"merged_list"}, set()), m_tlas_leaf_field: ({"tlas_leaf_fields"}, set()),
    m_leaf_alpha_tag: ({"leaf_alpha_tag"}, {"inner_alpha_tag", "cnode_child"}), m_empty_slot_box: ({"empty_slot"}, set()),
    m_ref_out_of_range: ({"ref_range"}, {"node_reach", "node_count", "leaf_permutation", "cnode_child", "inner_box", "inner_alpha_tag"}),
    m_single_child: ({"node_arity"}, CN | {"leaf_permutation", "inner_box", "inner_alpha_tag"}),
    m_stale_node_count: ({"node_count"}, {"node_reach"}),
    m_active_list: ({"active_list"}, set()), m_active_count: ({"active_list"}, set()), m_inst_pad: ({"inst_pad"}, set()),
    m_bvh2_root: ({"bvh2_root"}, set()), m_shade_tris: ({"shade_tris_ids"}, set()),
}


@pytest.mark.parametrize("mutate", list(MUTATIONS), ids=lambda f: f.__name__[2:])
def test_planted_defect_lights_its_own_check(clean, mutate):
    S, flat, two = clean
    flat, two = copy.deepcopy(flat), copy.deepcopy(two)
    mutate(S, flat, two)
    must, may = MUTATIONS[mutate]
    lit = set(A.failing(A.audit(flat, S))) | set(A.failing(A.audit(two, S)))
    assert must <= lit, f"{mutate.__name__}: {sorted(must - lit)} did not report it (lit: {sorted(lit)})"
    assert lit <= must | may, f"{mutate.__name__}: checks that do not cover the mutated element lit up: {sorted(lit - must - may)}"


def _unproven(checks, mutations):
    return sorted(set(checks) - set().union(*(must for must, _ in mutations.values())))


def test_every_check_has_a_planted_defect():
    assert _unproven(A.CHECKS, MUTATIONS) == []
    # ... and the rule bites: a check added to the auditor without its proof is named
    assert _unproven(A.CHECKS + ["a_new_check"], MUTATIONS) == ["a_new_check"]
    # a report can only carry the names of the list
    with pytest.raises(AssertionError):
        A._Report().add("a_new_check", np.zeros((1, 3), np.int64))

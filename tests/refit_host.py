"""The host build of the refit (csrc/pt_refit.h through tests/cpp/refit_host.cpp) and what its tests share: the deformation, the tables a dump's
hierarchies give the pure function, the function applied to a dump.  A plain module: no test lives here."""
import ctypes as C
import copy

import numpy as np

from tests import accel_audit as A
from tests import host_harness as H

U, F = np.uint32, np.float32
_P, _U = C.c_void_p, C.c_uint32
REFIT = H.StageLibrary("librefithost", "refit_host.cpp", [
    ("rfh_refit", C.c_int, [_U, _P, _U, _P, _P, _U, _P, _U, _P, _U, _P, _U, _P, _U, _P, _P, _U, _P, _P, _P])])
RF_WORLD, RF_VERTEX = 0, 1


def scene_lib():
    """the unit that writes a refitted structure into a harness scene; compiled with the harness's own scene header"""
    path = H.build_library("librefitscene", ["refit_scene_host.cpp"])
    return H.bind(path, [("rfh_scene_set_flat", C.c_int, [_P, _U, _P, _U, _P, _U, _P, _P, _P]), ("rfh_scene_set_two", C.c_int, [_P, _U, _P, _U, _P, _P, _P, _U, _P])])


def deform(scene, seed, sigma=0.25, only_mesh=None):
    """a copy of the finalized scene with an independent normal(0, sigma) on every position component and a second seeded offset on the texcoords
    (the handedness bit in texcoord[1]'s LSB moves with it: the whole record is what pt_update_vertices replaces); only_mesh: that prim-mesh's
    vertex range alone.  -> the copy, (first, count) of the vertices that changed"""
    from vk_raytrace_amd import capi
    if scene.vertices is None:
        scene.finalize(capi.pack_vertices)
    out = copy.copy(scene)
    v = np.array(scene.vertices, copy=True)
    first, count = 0, len(v)
    if only_mesh is not None:
        first, count = scene.prim_meshes[only_mesh][0], scene.prim_meshes[only_mesh][1]
    rng = np.random.default_rng(seed)
    v["position"][first:first + count] += rng.normal(0, sigma, (count, 3)).astype(F)
    v["texcoord"][first:first + count] += np.random.default_rng(seed + 1).normal(0, 0.125, (count, 2)).astype(F)
    out.vertices = v
    return out, (first, count)


def tables(dump, S):
    """node ranges and slot ranges (RfSlots words) of the hierarchies a refit keeps, from a dump and the scene inputs it was built from"""
    info, I = dump["info"], S["inst"]
    if info["accelMode"] == 0:
        return np.array([[0, info["numWideNodes"]]], U), np.array([[0, info["numTris"], RF_WORLD, 0, 0]], U)
    ranges, slots = [], []
    if info["mergedTris"]:
        ranges.append([0, info["mergedWide"]])
        slots.append([0, info["mergedTris"], RF_WORLD, 0, 0])
    hier = A._hierarchies(dump)
    R = dump.get("BLAS_RANGES")
    Lf = dump.get("TLAS_LEAVES")
    for k, (base, num) in enumerate(np.zeros((0, 2), U) if R is None else R):
        s0, n = A._blas_slots(hier[f"blas{k}"])
        inst = Lf[(Lf[:, 1] == base) & (Lf[:, 0] != A.PT_INST_MERGED), 0]
        assert len(inst), f"no TLAS leaf names the BLAS at node {base}"
        i = int(inst[0])
        assert n == I["triCount"][i]
        ranges.append([base, num])
        slots.append([s0, n, RF_VERTEX, I["vertexOffset"][i], I["firstIndex"][i]])
    order = np.argsort([s[0] for s in slots], kind="stable")
    return np.array(ranges, U).reshape(-1, 2), np.array(slots, U)[order].reshape(-1, 5)


def refit_dump(dump, S_built, S_new):
    """rfh_refit applied to a dump -> (a new dump with WIDE, TRIS, ALPHA_RECS, CNODES, SHADE_TRIS refitted and the merged box set, root boxes per node range,
    (costBefore, costAfter)).  S_built: the inputs the dump was built from (they say which mesh a BLAS holds); S_new: the deformed inputs"""
    L = REFIT.lib()
    ranges, slots = tables(dump, S_built)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dump.items()}
    out["info"] = dict(dump["info"])
    W, T, Al = out["WIDE"], out["TRIS"], out["ALPHA_RECS"]
    cn = out.get("CNODES") if dump["info"]["haveCNodes"] else None
    sh = out.get("SHADE_TRIS") if dump["info"]["haveShadeTris"] else None
    inst = np.ascontiguousarray(S_new["inst"])
    v, idx = np.ascontiguousarray(S_new["vertices"], F), np.ascontiguousarray(S_new["indices"], U)
    boxes, costs = np.zeros((len(ranges), 6), F), np.zeros(2, np.float64)
    rc = L.rfh_refit(len(W), W.ctypes.data, len(T), T.ctypes.data, Al.ctypes.data, len(ranges), ranges.ctypes.data, len(slots), slots.ctypes.data, len(inst), inst.ctypes.data,
                     len(v), v.ctypes.data, len(idx), idx.ctypes.data, None if cn is None else cn.ctypes.data, 0 if sh is None else len(sh), None if sh is None else sh.ctypes.data,
                     boxes.ctypes.data, costs.ctypes.data)
    assert rc == 0, f"rfh_refit refused its input: {rc}"
    if dump["info"]["accelMode"] != 0 and dump["info"]["mergedTris"]:
        out["info"]["mergedBox"] = boxes[0].copy()
        for k in range(6):
            out["info"][f"mbox{k}"] = int(boxes[0, k:k + 1].view(U)[0])
    return out, boxes, (float(costs[0]), float(costs[1]))


def used_boxes_all_changed(before, after):
    """every used child box of every reached node differs from its value before the refit in at least one plane; -> number of boxes looked at"""
    n = 0
    for name, h in A._hierarchies(before).items():
        if name == "tlas":
            continue
        levels, _, _ = A._walk(h, A._Report())
        nodes = np.concatenate(levels) if levels else np.zeros(0, np.int64)
        used = before["WIDE"][nodes, 24:28] != A.BVH_NONE
        planes_b = before["WIDE"][nodes, 0:24].reshape(-1, 6, 4)
        planes_a = after["WIDE"][nodes, 0:24].reshape(-1, 6, 4)
        same = (planes_b == planes_a).all(1)
        assert not (used & same).any(), (name, nodes[np.nonzero(used & same)[0]][:8])
        n += int(used.sum())
    return n

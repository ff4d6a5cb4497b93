"""The host build of the gather query: vk_raytrace_amd/csrc/pt_gather.h (gather_point<TWO, KIND>, what pt_gather's kernel runs per lane; DESIGN.md section
3.3) compiled by g++ from tests/cpp/gather_host.cpp into a library of its own next to the units of the host harness and the host build of the path query
(tests/cpp/paths_host.cpp: the composition tests feed the gather's rays through ph_paths of the SAME library), and its Python side: the binding, the
scene wrapper, and the points the host tests (tests/test_gather_host.py) and the device tests that take this build as their reference
(tests/test_gather_gpu.py) share.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import host_harness, paths_host
from vk_raytrace_amd import capi, host_device as hd

_P, _I, _U = C.c_void_p, C.c_int, C.c_uint32
NAME = "libgatherhost"
# tests/cpp/gather_host.cpp: (name, restype, argtypes)
SIGNATURES = [
    ("gh_gather", _U, [_P, _I, C.POINTER(hd.RtxState), _I, _U, C.c_uint64, _P, _P]),    # (scene, two, state, variant, kind, n, points, results) -> overflows
    ("gh_gather_rays", _U, [_P, _I, C.POINTER(hd.RtxState), _I, _U, _P, _P, _U]),       # (scene, two, state, variant, kind, point, rays out[cap], cap) -> rays
]
HEMISPHERE, SPHERE = capi.PT_GATHER_HEMISPHERE, capi.PT_GATHER_SPHERE
RESULT_DTYPE = {HEMISPHERE: hd.gatherresult_dtype, SPHERE: hd.proberesult_dtype}
_lib = None


def build():
    """tests/cpp/_build/libgatherhost.so: the harness's units, paths_host.cpp and gather_host.cpp (the Scene of th_scene.h is one struct in all of them)"""
    return host_harness.build_library(NAME, host_harness.UNITS + ["paths_host.cpp", "gather_host.cpp"], needs_libptmi=True)


def lib():
    global _lib
    if _lib is None:
        _lib = host_harness.bind(build(), host_harness.SIGNATURES + paths_host.SIGNATURES + SIGNATURES)
    return _lib


def make_points(positions, normals=None, seeds=None):
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    pts = np.zeros(len(p), hd.gatherpoint_dtype)
    pts["position"] = p
    if normals is not None:
        pts["normal"] = np.asarray(normals, np.float32).reshape(-1, 3)
    pts["seed"] = 0 if seeds is None else np.asarray(seeds, np.uint32)
    return pts


def surface_points(scene, n, rng):
    """n points on the scene's triangles: the centroid of a triangle drawn at random and its shading normal there (the mean of the three vertex
    normals, by the inverse transpose of the node's matrix), in world space; triangles of zero area or with a zero normal are passed over"""
    if scene.vertices is None:
        scene.finalize(capi.pack_vertices)
    pos = np.asarray(scene.vertices["position"], np.float64)
    nrm = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in scene._nrm])   # (the normals as given: the vertex records hold them packed)
    idx = np.asarray(scene.indices, np.int64)
    P, N = [], []
    nodes = [(np.asarray(m, np.float64), pm) for m, pm in scene.nodes if scene.prim_meshes[pm][3] >= 3]
    while len(P) < n:
        m, pm = nodes[rng.integers(len(nodes))]
        vo, vc, fi, ic, _ = scene.prim_meshes[pm]
        t = int(rng.integers(ic // 3))
        v = pos[vo + idx[fi + 3 * t:fi + 3 * t + 3]]
        w = v @ m[:3, :3].T + m[:3, 3]
        g = np.cross(w[1] - w[0], w[2] - w[0])
        if not np.linalg.norm(g) > 1e-12:
            continue
        s = np.linalg.inv(m[:3, :3]).T @ nrm[vo + idx[fi + 3 * t:fi + 3 * t + 3]].mean(0)
        g = s if np.linalg.norm(s) > 1e-6 else g
        P.append(w.mean(0)); N.append(g / np.linalg.norm(g))
    return np.array(P, np.float32), np.array(N, np.float32)


def scene_points(scene, rng, on_surface=257, free=64):
    """the point set of the tests: `on_surface` points on triangles and `free` points in the scene's bounding box with random normals of random
    length, each with a seed of its own: hd.gatherpoint_dtype records"""
    p, nrm = surface_points(scene, on_surface, rng)
    lo, hi = p.min(0), p.max(0)
    fp = rng.uniform(lo, hi, (free, 3)).astype(np.float32)
    fn = (rng.normal(0, 1, (free, 3)) * 10.0 ** rng.uniform(-2, 2, (free, 1))).astype(np.float32)
    n = on_surface + free
    return make_points(np.concatenate([p, fp]), np.concatenate([nrm, fn]), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))


class GatherScene(paths_host.PathScene):
    """paths_host.PathScene on this module's library: cfg on the harness with environment, camera and sun & sky installed; paths() is the host build of
    section 3.2 (ph_paths), gather() the host build of section 3.3"""

    def __init__(self, cfg):
        self.cfg, self.L = cfg, lib()
        self.tr = host_harness.TracedScene(cfg.scene)
        integral = C.c_float()
        assert self.L.th_set_env(self.tr.h, cfg.env.ctypes.data, cfg.env.shape[1], cfg.env.shape[0], C.byref(integral)) == 0
        self.L.th_set_camera(self.tr.h, C.byref(cfg.camera), C.byref(cfg.sunsky))
        self.integral = integral.value

    def gather(self, two, st, kind, points, variant=None, overflow=False):
        """gather_point on the host: (n,) records of the kind's type.  overflow: also return the traversal-stack overflows"""
        points = np.ascontiguousarray(points, hd.gatherpoint_dtype)
        out = np.zeros(len(points), RESULT_DTYPE[int(kind)])
        over = self.L.gh_gather(self.tr.h, int(two), C.byref(st), self.cfg.variant if variant is None else int(variant), int(kind), len(points), points.ctypes.data, out.ctypes.data)
        if overflow:
            return out, over
        assert over == 0, "traversal stack overflow"
        return out

    def rays(self, two, st, kind, point, variant=None):
        """the (origin, direction, seed at the start of the path) of every sample of one point, in sample order: hd.ray_dtype records (none for an
        invalid point)"""
        one = np.ascontiguousarray(point, hd.gatherpoint_dtype).reshape(1)
        out = np.zeros(st.maxSamples, hd.ray_dtype)
        n = self.L.gh_gather_rays(self.tr.h, int(two), C.byref(st), self.cfg.variant if variant is None else int(variant), int(kind), one.ctypes.data, out.ctypes.data, len(out))
        assert n in (0, len(out))
        return out[:n]

"""The host harness of the trace source: the product's own headers (vk_raytrace_amd/csrc/pt_trace.h, pt_machine.h, pt_settle.h, pt_shade.h, pt_probe.h,
pt_query.h) compiled for the host by g++ from the units under tests/cpp/, and its Python side -- the one build function (build_library, which the host
builds of the display stages' headers go through as well: tests/denoise_host.py, guides_host.py, temporal_host.py, svgf_host.py), the one binder of
ctypes signature tables, the scene wrappers (Traced, TracedScene, host_render) and the scenes and rays the host tests, the device tests that take the
host build as their reference, and the CPU experiments under tools/ share.  A plain module: no test lives here."""
import concurrent.futures
import ctypes as C
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

from vk_raytrace_amd import capi, synth
from vk_raytrace_amd.scene import Scene, translate, scale, rotate_x, rotate_y, rotate_z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD_DIR = os.path.join(CPP, "_build")
NONE = 0xFFFFFFFF
OPAQUE, NOCULL = 1, 2
MERGE_SINGLES, COMPACT_NODES = 1, 2   # the options word of th_create / th_create_scene (tests/cpp/th_scene.h)

# ---- the build ---------------------------------------------------------------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "vk_raytrace_amd", "csrc")
# what every host build of a product header is compiled with: the device build's floating-point contract
COMPILE = ["-std=c++17", "-O2", "-fopenmp", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DSTACK_LDS=24", "-Wno-attributes",
           "-I/opt/rocm/include", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
UNITS = ["trace_host.cpp", "render_host.cpp", "probe_host.cpp", "query_host.cpp", "handover_host.cpp"]
# flavour -> (extra compiler flags, extra units).  "" is what every test uses; the others carry the experiments of tools/ (tests/cpp/experiments/)
FLAVOURS = {"": ([], []), "steps": ([], ["experiments/step_model.cpp"]), "robust": (["-DTH_ROBUST_T2"], ["experiments/t2_experiment.cpp"]),
            "certified": (["-DTH_CERTIFIED_T2"], ["experiments/t2_experiment.cpp"])}
JOBS = 8   # units compiled at a time: fixed, not the machine's CPU count


def _gxx(args):
    subprocess.check_call(["g++"] + args)


def _project_deps(dfile):
    """the files of this repository among the prerequisites g++ -MMD wrote (system and ROCm headers are left out), relative to its root"""
    words = open(dfile).read().replace("\\\n", " ").split()
    paths = {os.path.realpath(w) for w in words if not w.endswith(":")}
    root = os.path.realpath(ROOT) + os.sep
    return sorted(os.path.relpath(p, root) for p in paths if p.startswith(root))


def build_library(name, units, flags=(), needs_libptmi=False):
    """tests/cpp/_build/<name>.so from the units (paths under tests/cpp/), compiled if it is missing or older than any project file the compiler read
    for it, or if the recipe changed; returns its path.  The list of those files is kept next to it (<library>.json).  needs_libptmi: the library
    links libptmi.so's host-side test hooks -- that must exist then, and a newer one rebuilds; without it nothing of the product need be built."""
    out = os.path.join(BUILD_DIR, name + ".so")
    compile_args, link_args, newer = COMPILE + list(flags), ["-shared", "-fopenmp"], []
    if needs_libptmi:
        capi.lib()
        lib_dir = os.path.dirname(capi.LIB_PATH)
        link_args += ["-L" + lib_dir, "-l:libptmi.so", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
        newer = [capi.LIB_PATH]
    recipe = {"units": list(units), "compile": compile_args, "link": link_args}
    try:
        stamp = json.load(open(out + ".json"))
        built = os.path.getmtime(out)
        if stamp["recipe"] == recipe and all(os.path.getmtime(f) <= built for f in [os.path.join(ROOT, d) for d in stamp["deps"]] + newer):
            return out
    except (OSError, ValueError, KeyError):
        pass
    os.makedirs(BUILD_DIR, exist_ok=True)
    tmp = tempfile.mkdtemp(dir=BUILD_DIR)   # ranks that build at the same time each work in a directory of their own ...
    try:
        objs = [os.path.join(tmp, u.replace("/", "_") + ".o") for u in recipe["units"]]
        with concurrent.futures.ThreadPoolExecutor(JOBS) as pool:
            list(pool.map(lambda uo: _gxx(compile_args + ["-MMD", "-c", os.path.join(CPP, uo[0]), "-o", uo[1]]), zip(recipe["units"], objs)))
        _gxx(objs + link_args + ["-o", os.path.join(tmp, "lib.so")])
        deps = sorted(set().union(*(_project_deps(o[:-2] + ".d") for o in objs)))
        with open(os.path.join(tmp, "lib.json"), "w") as f:
            json.dump({"recipe": recipe, "deps": deps}, f, indent=1)
        os.replace(os.path.join(tmp, "lib.so"), out)   # ... and nobody ever loads a half-written file
        os.replace(os.path.join(tmp, "lib.json"), out + ".json")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def compile_to(out, unit, header_dir):
    """The one-unit library `out` with `header_dir` searched before csrc/ (a scratch copy of a header with a planted break); no cache, no record.
    csrc/'s other headers are copied next to it first: one that includes the broken header finds it in its own directory, which must be the scratch one"""
    for name in os.listdir(CSRC):
        if name.endswith(".h") and not os.path.exists(os.path.join(header_dir, name)):
            shutil.copy(os.path.join(CSRC, name), header_dir)
    _gxx(["-I" + header_dir] + COMPILE + ["-shared", "-o", out, os.path.join(CPP, unit)])
    return out


def build(flavour=""):
    """libtracehost[_<flavour>].so (build_library); it links libptmi.so: the device-builder emulation, two_level_pad, the scene records"""
    flags, extra = FLAVOURS[flavour]
    return build_library("libtracehost" + ("_" + flavour if flavour else ""), UNITS + extra, flags, needs_libptmi=True)


def bind(path, signatures):
    """the library at `path` with every (name, restype, argtypes) of the table applied; a name that does not resolve is an error"""
    L = C.CDLL(path)
    for name, restype, argtypes in signatures:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


class StageLibrary:
    """the host build of one stage header: a one-unit library that needs no libptmi.so, and its signature table"""
    def __init__(self, name, unit, signatures):
        self.name, self.unit, self.signatures, self._lib = name, unit, signatures, None

    def build(self):
        return build_library(self.name, [self.unit])

    def compile_to(self, out, header_dir):
        return compile_to(out, self.unit, header_dir)

    def bind(self, path):
        return bind(path, self.signatures)

    def lib(self):
        if self._lib is None:
            self._lib = self.bind(self.build())
        return self._lib


def planes_arg(guides, h, w):
    """three guide planes (None: not installed) as the host builds take them: (the arrays to keep alive, a void*[3])"""
    keep = [None if g is None else np.ascontiguousarray(g, np.float32) for g in (guides or (None, None, None))]
    assert len(keep) == 3 and all(g is None or g.shape == (h, w, 4) for g in keep)
    return keep, (C.c_void_p * 3)(*[None if g is None else g.ctypes.data for g in keep])


def deps(path=None):
    """the project files build_library recorded for the library at `path` (None: the trace library, built if need be), relative to the repository's root"""
    return json.load(open((path or build()) + ".json"))["deps"]


# ---- the entry points: (name, restype, argtypes) -----------------------------------------------------------------------------------------------------
_P, _I, _U = C.c_void_p, C.c_int, C.c_uint32
_PROBE = [_I, C.c_uint64, _P, _I, _P, _I]   # csrc/pt_probe.h: (fn or kind, n, in, in_stride, out, out_stride)
SIGNATURES = [
    # tests/cpp/trace_host.cpp
    ("th_create", _P, [_P, _U, _P, _U, _P, _U, _P, _U, _U]),
    ("th_create_scene", _P, [_P, C.c_char_p, C.c_size_t, _U]),
    ("th_destroy", None, [_P]),
    ("th_num_tris", _U, [_P]),
    ("th_sizes", None, [_P, _P]),
    ("th_world_tri", None, [_P, _U, _P, _P]),
    ("th_compact_in_use", _I, [_P, _I]),
    ("th_compact_ok", _I, [_P]),
    ("th_cnode_violations", C.c_ulonglong, [_P, _P]),
    ("th_candidates", _U, [_P, _I, _U, _P, _P, C.c_float, _U, _P, _P]),
    ("th_settle", _U, [_P, _I, _I, _I, _I, _U] + [_P] * 8),
    ("th_take_sp_hist", None, [_P]),
    ("th_accel_info", _I, [_P, _I, _P, _I]),                            # csrc/pt_accel_dump.h: (scene, two, out[words], words)
    ("th_accel_read", C.c_longlong, [_P, _I, _I, _P, C.c_size_t]),      # (scene, two, array id, dst, bytes) -> bytes the array holds
    # tests/cpp/render_host.cpp
    ("th_set_env", _I, [_P, _P, _I, _I, _P]),
    ("th_set_camera", None, [_P, _P, _P]),
    ("th_render_shard", _U, [_P, _I, _P, _I, _I, _I, _I, _P]),
    # tests/cpp/probe_host.cpp
    ("th_shading_probe", _I, _PROBE),
    ("th_trace_probe", _I, _PROBE),
    ("th_texture_probe", _I, [_P] + _PROBE),
    ("th_surface_probe", _I, [_P] + _PROBE),
    ("th_texture_records", None, [_P] * 7),
    ("th_clear_fast_tap", None, [_P]),
    # tests/cpp/query_host.cpp, tests/cpp/handover_host.cpp
    ("qh_query", _U, [_P, _I, _I, _I, C.c_uint64, _P, _P, _U]),
    ("th_handover", _U, [_P, _I, _U] + [_P] * 6),
]
# entry points that exist in an experiment flavour only (tests/cpp/experiments/)
EXPERIMENT_SIGNATURES = {
    "steps": [("th_step_model", None, [_P, _I, _I, _U, _P, _P, _P, _P])],
    "robust": [("th_t2_stats", None, [_P])],
    "certified": [("th_t2_stats", None, [_P]), ("th_t2_accepts", C.c_ulonglong, [])],
}
_libs = {}


def lib(flavour=""):
    """the library of that flavour, built if need be, with every signature of the table applied"""
    if flavour not in _libs:
        _libs[flavour] = bind(build(flavour), SIGNATURES + EXPERIMENT_SIGNATURES.get(flavour, []))
    return _libs[flavour]


# ---- scenes on the harness ---------------------------------------------------------------------------------------------------------------------------
class InstIn(C.Structure):
    _fields_ = [("vertexOffset", C.c_uint32), ("firstIndex", C.c_uint32), ("triCount", C.c_uint32), ("flags", C.c_uint32), ("primMesh", C.c_int32), ("worldMatrix", C.c_float * 16)]


def _options(merge_singles, compact_nodes):
    return (MERGE_SINGLES if merge_singles else 0) | (COMPACT_NODES if compact_nodes else 0)


class Traced:
    def __init__(self, scene: Scene, flags, merge_singles=True, compact_nodes=False, flavour=""):
        """flags: per node TRI_OPAQUE | TRI_NOCULL bits.  merge_singles: the two-level structure keeps the prim-meshes instantiated once in one
        world-space structure (the product's default, PT_TUNE mergeSingles) or gives every prim-mesh its own object-space BLAS.  compact_nodes:
        the machine walks read the 80-byte form of the nodes (PT_TUNE cnodes)"""
        self.L = lib(flavour)
        if scene.vertices is None:
            scene.finalize(capi.pack_vertices)
        v = np.ascontiguousarray(scene.vertices)
        idx = np.ascontiguousarray(scene.indices, np.uint32)
        inst = (InstIn * len(scene.nodes))()
        for i, (m, pm) in enumerate(scene.nodes):
            vo, vc, fi, ic, _ = scene.prim_meshes[pm]
            inst[i] = InstIn(vo, fi, ic // 3, int(flags[i]), pm, (C.c_float * 16)(*np.asarray(m, np.float32).T.reshape(16)))
        bound = np.zeros(len(scene.prim_meshes), np.float32)
        for p, (vo, vc, fi, ic, _) in enumerate(scene.prim_meshes):
            bound[p] = np.abs(v["position"][vo:vo + vc]).max() if vc else 0.0
        self.h = self.L.th_create(v.ctypes.data, len(v), idx.ctypes.data, len(idx), C.addressof(inst), len(inst), bound.ctypes.data, len(bound), _options(merge_singles, compact_nodes))
        assert self.h, "th_create failed"
        self.keep = (v, idx, inst, bound)
        self.n = self.L.th_num_tris(self.h)

    def candidates(self, mode, org, dirs, tmax=1e32, max_cand=6):
        org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
        w = np.zeros((len(org), max_cand), np.uint32)
        t = np.zeros((len(org), max_cand), np.float32)
        over = self.L.th_candidates(self.h, mode, len(org), org.ctypes.data, dirs.ctypes.data, tmax, max_cand, w.ctypes.data, t.ctypes.data)
        assert over == 0, "traversal stack overflow"
        return w, t

    def world_tri(self, w):
        out = np.zeros(9, np.float32)
        fl = C.c_uint32()
        self.L.th_world_tri(self.h, int(w), out.ctypes.data, C.byref(fl))
        return out.astype(np.float64), fl.value

    def sizes(self):
        out = np.zeros(4, np.uint32)
        self.L.th_sizes(self.h, out.ctypes.data)
        return out

    def close(self):
        self.L.th_destroy(self.h)


class TracedScene(Traced):
    """a full scene description (materials, textures): instance flags, alpha view, opacity maps and texel pool come from the product's own
    host code (pt_scene_records.cpp build_scene_records)"""

    def __init__(self, scene: Scene, merge_singles=True, compact_nodes=False, flavour=""):
        self.L = lib(flavour)
        if scene.vertices is None:
            scene.finalize(capi.pack_vertices)
        d, keep = scene.desc()
        err = C.create_string_buffer(256)
        self.h = self.L.th_create_scene(C.byref(d), err, 256, _options(merge_singles, compact_nodes))
        assert self.h, err.value
        self.keep = keep
        self.n = self.L.th_num_tris(self.h)

    def settle(self, kind, two, exact, org, dirs, seeds, tmax=None, variant=0, sp_hist=False):
        """sp_hist: also return the histogram of the deepest traversal-stack level each trace-machine walk (exact = 2) used (bin 64: 64 or
        more) and the number of overflows (pushes beyond STACK_LDS + STACK_SPILL = 64 entries) instead of asserting that there are none"""
        org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
        seeds = np.ascontiguousarray(seeds, np.uint32)
        n = len(org)
        tm = None if tmax is None else np.ascontiguousarray(tmax, np.float32)
        w, tuv, sd, dr = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        hist = np.zeros(65, np.uint64)
        self.L.th_take_sp_hist(hist.ctypes.data)
        over = self.L.th_settle(self.h, kind, two, exact, variant, n, org.ctypes.data, dirs.ctypes.data, tm.ctypes.data if tm is not None else None, seeds.ctypes.data,
                                w.ctypes.data, tuv.ctypes.data, sd.ctypes.data, dr.ctypes.data)
        self.L.th_take_sp_hist(hist.ctypes.data)
        if sp_hist:
            return w, tuv, sd, dr, hist, over
        assert over == 0
        return w, tuv, sd, dr


# ---- whole frames ------------------------------------------------------------------------------------------------------------------------------------
def host_render(cfg, frames, two=0, shard=None):
    """cfg: tests.common.Config.  The frames k_generate / k_tail / k_accumulate would produce, computed by the same functions (pt_shade.h,
    pt_settle.h, pt_trace.h, pt_bsdf.h, pt_surface.h, pt_sky.h) compiled for the host.  shard = (rank, nranks): only that rank's image tiles
    (pt_set_shard), the other pixels stay zero."""
    tr = TracedScene(cfg.scene)
    L = tr.L
    integral = C.c_float()
    assert L.th_set_env(tr.h, cfg.env.ctypes.data, cfg.env.shape[1], cfg.env.shape[0], C.byref(integral)) == 0
    L.th_set_camera(tr.h, C.byref(cfg.camera), C.byref(cfg.sunsky))
    st = cfg.state(integral.value)
    out = np.zeros((cfg.height, cfg.width, 4), np.float32)
    rank, nranks = shard if shard is not None else (0, 1)
    assert L.th_render_shard(tr.h, two, C.byref(st), cfg.variant, frames, rank, nranks, out.ctypes.data) == 0
    tr.close()
    return out


# ---- scenes, rays and the rule for comparing candidate lists -----------------------------------------------------------------------------------------
def ill_conditioned(tr, o, d, t32):
    """Moeller-Trumbore in double precision on the fp32 inputs.  True when fp32's verdict on this triangle is an artefact of cancellation:
    the ray misses the triangle in exact arithmetic (an ACCIDENTAL hit), or the fp32 hit distance is off by more than the box tests'
    tolerance (the triangle is nearly edge-on: det ~ 0), so that pruning against it -- or it against another candidate -- depends on the
    order in which a walk meets them."""
    tri, _ = tr
    p0, e1, e2 = tri[0:3], tri[3:6], tri[6:9]
    o, d = o.astype(np.float64), d.astype(np.float64)
    pv = np.cross(d, e2)
    det = e1 @ pv
    if det == 0.0:
        return True
    tv = o - p0
    u = (tv @ pv) / det
    qv = np.cross(tv, e1)
    v = (d @ qv) / det
    t = (e2 @ qv) / det
    eps = 1e-9
    if u < -eps or v < -eps or u + v > 1 + eps:
        return True
    return abs(float(t32) - t) > 4e-7 * abs(t) + 1e-30


def instanced_scene(seed, n_nodes=160, far=False):
    rng = np.random.default_rng(seed)
    sc = Scene(f"trace{seed}")
    m = sc.add_material()
    meshes = [synth.uv_sphere(0.5, 16, 8), synth.box((0.8, 0.9, 0.7), sub=3), synth.revolve(0.2 + 0.1 * np.sin(np.linspace(0, 3, 9)), np.linspace(0, 1, 9), 12),
              synth.cards(rng, 40, (0, 0.5, 0), (0.8, 1.0, 0.8), 0.2), synth.grid(6, 6, (-1, 0, 1), (2, 0, 0), (0, 0, -2))]
    pms = [sc.add_prim_mesh(p, n, uv, i, m, tangents=t) for (p, n, uv, i, t) in meshes]
    tri = sc.add_prim_mesh([(-1, -1, 0), (1, -1, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [(0, 0), (1, 0), (0.5, 1)], [0, 1, 2], m)   # single-leaf BLAS
    hole = sc.add_prim_mesh(np.zeros((3, 3)), [(0, 0, 1)] * 3, np.zeros((3, 2)), np.zeros(0, np.uint32), m)                      # no triangles
    flags = []
    off = np.array([3000.0, -1500.0, 800.0]) if far else np.zeros(3)
    for i in range(n_nodes):
        s = 10.0 ** rng.uniform(-0.7, 0.7, 3) if i % 3 else np.full(3, 10.0 ** rng.uniform(-0.5, 0.5))
        if i % 7 == 0:
            s[rng.integers(3)] *= -1.0   # mirrored
        t = rng.uniform(-6, 6, 3) + off
        mtx = translate(*t) @ rotate_y(rng.uniform(0, 6.3)) @ rotate_x(rng.uniform(0, 6.3)) @ rotate_z(rng.uniform(0, 6.3)) @ scale(*s)
        if i % 11 == 0:
            mtx = translate(*t)          # axis-aligned instances: boxes whose faces are parallel to axis-parallel rays
        pm = (pms + [tri, hole])[i % 7]
        sc.add_node(pm, mtx)
        flags.append(OPAQUE | (NOCULL if i % 2 else 0))
    # two instances of the same mesh exactly on top of each other: ties in t across instances
    mtx = translate(*(np.array([0.5, 0.5, 0.5]) + off))
    sc.add_node(pms[1], mtx); flags.append(OPAQUE | NOCULL)
    sc.add_node(pms[1], mtx); flags.append(OPAQUE | NOCULL)
    # prim-meshes with ONE instance each (the two-level structure keeps these in its merged world-space structure): rotated + non-uniformly
    # scaled, mirrored, and one overlapping the coincident pair above
    once = [sc.add_prim_mesh(p, n, uv, i, m, tangents=t) for (p, n, uv, i, t) in (synth.uv_sphere(0.7, 12, 6), synth.box((1.1, 0.6, 0.9), sub=2), synth.grid(4, 4, (-1, 0, 1), (2, 0, 0), (0, 0, -2)))]
    sc.add_node(once[0], translate(*(np.array([-2.0, 1.0, 3.0]) + off)) @ rotate_y(0.7) @ rotate_x(1.9) @ scale(1.5, 0.4, 2.2)); flags.append(OPAQUE)
    sc.add_node(once[1], translate(*(np.array([0.6, 0.4, 0.5]) + off)) @ rotate_z(0.3) @ scale(-1.0, 1.0, 1.0)); flags.append(OPAQUE | NOCULL)
    sc.add_node(once[2], translate(*(np.array([1.0, -2.0, -1.0]) + off)) @ rotate_x(0.4) @ scale(3.0, 1.0, 3.0)); flags.append(OPAQUE | NOCULL)
    return sc, np.array(flags), off


def rays_for(tr: Traced, rng, off, n):
    """camera-like, surface-to-surface, axis-parallel and far-origin rays"""
    org, dirs = [], []
    # towards random triangles from a ring of eye points
    k = n // 4
    targets = rng.integers(0, tr.n, k)
    pts = []
    for w in targets:
        tri, _ = tr.world_tri(w)
        b = rng.dirichlet((1, 1, 1))
        pts.append(tri[0:3] + b[1] * tri[3:6] + b[2] * tri[6:9])
    pts = np.array(pts)
    eye = off + rng.normal(0, 1, (k, 3)) * 14.0
    org.append(eye); dirs.append(pts - eye)
    # between surface points (what a bounce ray is), started a few ulps off the surface
    a, b = pts[rng.permutation(k)], pts[rng.permutation(k)]
    org.append(a + (b - a) * 1e-6); dirs.append(b - a)
    # axis-parallel rays through the scene, some exactly through lattice-like coordinates
    o = off + np.round(rng.uniform(-7, 7, (k, 3)) * 2) / 2
    ax = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1))
    org.append(o - ax * 20); dirs.append(ax)
    # from far outside
    o = off + rng.normal(0, 1, (n - 3 * k, 3)) * 3000.0
    org.append(o); dirs.append(pts[rng.integers(0, k, n - 3 * k)] - o)
    org, dirs = np.concatenate(org), np.concatenate(dirs)
    dirs = dirs / np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-30)
    return org.astype(np.float32), dirs.astype(np.float32)


def accidental_differences(tr, org, dirs, ref_w, ref_t, w, t, what):
    """candidate lists (n, k) against their reference: a ray that differs is accepted only when fp32's verdict on one of the two triangles at the
    first differing position -- one side reports a triangle the other skips -- is an artefact (ill_conditioned); a well-conditioned hit that a
    walk loses is a hole in its box tests.  Returns how many rays were accepted that way."""
    differs = (w != ref_w) | (np.ascontiguousarray(t, np.float32).view(np.uint32) != np.ascontiguousarray(ref_t, np.float32).view(np.uint32))
    bad = np.nonzero(differs.any(1))[0]
    for r in bad:
        c = int(np.nonzero(differs[r])[0][0])
        involved = [(ref_w[r, c], ref_t[r, c]), (w[r, c], t[r, c])]
        assert any(x != NONE and ill_conditioned(tr.world_tri(x), org[r], dirs[r], tx) for x, tx in involved), \
            f"{what}: ray {r} candidate {c}: reference {ref_w[r]} {ref_t[r]} vs {w[r]} {t[r]}"
    return len(bad)


def compare(tr, org, dirs, what, max_cand=6):
    """both walks against brute force -> (brute-force candidates, rays accepted as accidental differences)"""
    ref_w, ref_t = tr.candidates(0, org, dirs, max_cand=max_cand)
    accidental = sum(accidental_differences(tr, org, dirs, ref_w, ref_t, *tr.candidates(mode, org, dirs, max_cand=max_cand), f"{what}, {name}") for mode, name in ((1, "flat"), (2, "two-level")))
    return int((ref_w != NONE).sum()), accidental


def scene_rays(tr, rng, n, eye_center, eye_spread):
    k = n // 2
    targets = rng.integers(0, tr.n, n)
    pts = []
    for w in targets:
        tri, _ = tr.world_tri(w)
        b = rng.dirichlet((1, 1, 1))
        pts.append(tri[0:3] + b[1] * tri[3:6] + b[2] * tri[6:9])
    pts = np.array(pts)
    eye = np.asarray(eye_center) + rng.normal(0, 1, (k, 3)) * eye_spread
    a, b = pts[:n - k], pts[rng.permutation(n)[:n - k]]
    org = np.concatenate([eye, a + (b - a) * 1e-5])
    dirs = np.concatenate([pts[:k] - eye, b - a])
    dirs = dirs / np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-30)
    return org.astype(np.float32), dirs.astype(np.float32)


def alpha_scenes():
    yield "fuzz0", synth.fuzz_scene(0), (0, 0, 6), 3.0
    yield "fuzz1", synth.fuzz_scene(1), (0, 0, 6), 3.0
    yield "fuzz5", synth.fuzz_scene(5), (0, 0, 6), 3.0
    yield "sponza-like", synth.sponza_like(target_tris=12000, tex_size=64), (0, 3, 0), 4.0   # foliage cards: MASK with power-of-two textures -> opacity maps


def deep_rays(cfg):
    """camera rays through the pixel centres of cfg (pinhole)"""
    from vk_raytrace_amd.scene import Camera
    cam: Camera = cfg.scene.camera
    t = np.tan(np.radians(cam.fov) / 2)
    ys, xs = np.mgrid[0:cfg.height, 0:cfg.width]
    d = np.stack([(2 * (xs + 0.5) / cfg.width - 1) * t * cfg.width / cfg.height, (1 - 2 * (ys + 0.5) / cfg.height) * t, np.ones(xs.shape)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(cam.eye, np.float64), d.shape)
    return o, d


def camera_rays(cam, rng, n):
    """n rays from the camera through uniformly random points of a 16:9 image plane (what the experiments under tools/ walk)"""
    eye = np.array(cam.eye, np.float64)
    fwd = np.array(cam.center, np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array(cam.up, np.float64)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    th = np.tan(np.radians(cam.fov) / 2)
    px = rng.uniform(-1, 1, (n, 2)) * (th * 16 / 9, th)
    d = fwd + px[:, :1] * right + px[:, 1:] * up
    return np.repeat(eye[None], n, 0), d / np.linalg.norm(d, axis=1, keepdims=True)

"""Shared by tests/test_surface_model.py and tests/golden/measure_surface_kat.py: the fixture of tests/golden/gen_surface_kat.py, the scene it describes, and
the surface probes (vk_raytrace_amd/csrc/pt_probe.h surface_probe: th_surface_probe on the host build, pt_debug_surface_probe on the device,
orc_surface_probe on the oracle, ref_surface_probe on the compiled reference).  A probe takes rows of IN words and fills rows of OUT words; integers
travel as bit patterns; rows a probe refuses keep the caller's fill."""
import importlib.util
import os

import numpy as np

from vk_raytrace_amd import host_device as hd
from vk_raytrace_amd.scene import Camera, Scene, Texture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE, SLOT = 0, 1
IN, OUT, WORDS = 8, 72, 69
LINE_WORD = 68          # 1 when the product shaded the material from its 128-byte line alone
INT_WORDS = (65, 66, 67)
NO_DATA = 1


def generator():
    spec = importlib.util.spec_from_file_location("gen_surface_kat", os.path.join(GOLDEN, "gen_surface_kat.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def load(path=None):
    with np.load(path or os.path.join(GOLDEN, "surface_kat.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_scene(kat):
    """the fixture's arrays as a Scene: the packed vertices are written word for word (the codes are the fixture's, not a packer's), the prim-mesh records
    alias the five pieces of geometry, one record per material"""
    sc = Scene("surface fixture")
    v = np.zeros(len(kat["position"]), hd.vertex_dtype)
    v["position"], v["normal"], v["texcoord"], v["tangent"], v["color"] = kat["position"], kat["normal_code"], kat["texcoord"], kat["tangent_code"], kat["color_code"]
    sc.vertices, sc.indices = v, kat["indices"].astype(np.uint32)
    sc.prim_meshes = [tuple(int(x) for x in r) for r in kat["records"]]
    assert kat["materials"].dtype.itemsize == hd.material_dtype.itemsize
    sc.materials = list(np.frombuffer(kat["materials"].tobytes(), hd.material_dtype).copy())
    for t, (mag, ws, wt) in enumerate(kat["tex_sampler"]):
        sc.textures.append(Texture(np.ascontiguousarray(kat[f"tex{t}"]), magFilter=int(mag), minFilter=int(mag), wrapS=int(ws), wrapT=int(wt)))
    sc.nodes = [(np.asarray(m, np.float32), int(r)) for m, r in zip(kat["node_matrix"], kat["node_record"])]
    sc.camera = Camera(eye=(0.0, 0.0, 25.0), center=(0.0, 0.0, 0.0), fov=50.0)   # the records lie side by side around the origin, 3 apart
    return sc


def probe_rows(kat, path=0, sel=None):
    n = len(kat["row_inst"])
    r = np.zeros((n, IN), np.float32)
    u = r.view(np.uint32)
    u[:, 0], u[:, 1], u[:, 7] = kat["row_inst"], kat["row_prim"], path
    r[:, 2], r[:, 3], r[:, 4:7] = kat["row_bu"], kat["row_bv"], kat["row_dir"]
    return r if sel is None else np.ascontiguousarray(r[sel])


def call(fn, args, kind, r, fill=np.nan):
    """rows through one call -> ((n, OUT) float32, the call's code)"""
    r = np.ascontiguousarray(r, np.float32)
    out = np.full((len(r), OUT), fill, np.float32)
    rc = fn(*args, kind, len(r), r.ctypes.data, r.shape[1], out.ctypes.data, OUT)
    return out, rc


class HostScene:
    """the product's headers compiled for the host (tests/cpp/trace_host.cpp) on the product's own records of the scene, under one PT_TUNE setting"""

    def __init__(self, scene, tune=None):
        from tests import tex_kat_io
        self.hs = tex_kat_io.HostScene(scene, tune)

    def probe(self, kind, r, fill=np.nan):
        out, rc = call(self.hs.L.th_surface_probe, (self.hs.h,), kind, r, fill)
        assert rc in (0, NO_DATA), rc
        return out, rc

    def close(self):
        self.hs.close()


def oracle_probe(o, kind, r, fill=np.nan):
    return call(o.L.orc_surface_probe, (o.ctx,), kind, r, fill)


def reference_probe(ref, kind, r, fill=np.nan):
    return call(ref.L.ref_surface_probe, (), kind, r, fill)


def values(out):
    """a probe's output as float64 values, the integer words read as integers"""
    v = out[:, :WORDS].astype(np.float64)
    for w in INT_WORDS + (LINE_WORD,):
        v[:, w] = out[:, w].view(np.uint32)
    return v


def errors(kat, out, rows=None):
    """per group the largest |got - want| / max(1, |want|) over the given rows (default: the kept ones) -> {group: error}"""
    rows = kat["row_kept"] if rows is None else rows
    want, got = kat["want"].T[rows], values(out)[rows]
    res = {}
    for name, (first, count) in zip(kat["group_names"], kat["group_words"]):
        w, g = want[:, first:first + count], got[:, first:first + count]
        with np.errstate(invalid="ignore"):
            e = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        e[np.isnan(e)] = np.inf
        res[str(name)] = float(e.max()) if e.size else 0.0
    return res


def same_bits(a, b):
    """NaN in the same places, every other value equal as bits; returns the number of differing values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero(an != bn) + np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~an & ~bn))

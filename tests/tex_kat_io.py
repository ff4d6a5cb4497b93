"""Shared by tests/test_texture_model.py: the fixture of tests/golden/gen_tex_kat.py, the scene that carries its textures, and the texture probes
(vk_raytrace_amd/csrc/pt_probe.h texture_probe: th_texture_probe on the host build, pt_debug_texture_probe on the device).  A probe takes
(scene or context, kind, n, in, in_stride, out, out_stride) with rows of IN words in and OUT words out; integers travel as bit patterns."""
import contextlib
import ctypes as C
import importlib.util
import os

import numpy as np

from vk_raytrace_amd import capi
from vk_raytrace_amd.scene import Scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAP, SAMPLE_REC, SAMPLE_DESC, OPACITY, ENV, WRAP, INDEX, DESC = range(8)
IN, OUT = 12, 8
CONFIGS = 18
BASE_SLOT = 3   # a material line holds the descriptors of its normal, emissive, metallic-roughness and base-colour texture, in that order
TUNES = (None, "texTile=0", "texGroups=0", "texTile=0,texGroups=0")   # the four storage settings


def generator():
    spec = importlib.util.spec_from_file_location("gen_tex_kat", os.path.join(GOLDEN, "gen_tex_kat.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def load():
    with np.load(os.path.join(GOLDEN, "tex_kat.npz")) as z:
        return {k: z[k] for k in z.files}


@contextlib.contextmanager
def tuned(tune):
    """PT_TUNE for the scene records made inside the block (pt_debug_scene_records and pt_create read it when they are called)"""
    old = os.environ.get("PT_TUNE")
    if tune is None:
        os.environ.pop("PT_TUNE", None)
    else:
        os.environ["PT_TUNE"] = tune
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("PT_TUNE", None)
        else:
            os.environ["PT_TUNE"] = old


def add_quad(sc, material, z=0.0):
    pm = sc.add_prim_mesh([(-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)], [(0, 0, 1)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)], [0, 1, 2, 0, 2, 3], material)
    sc.add_node(pm)


def fixture_scene(kat):
    """texture id = fixture texture x 18 + config (wrapS, wrapT, filter); material id = texture id, the texture in the base-colour role"""
    sc = Scene("texture fixture")
    for t in range(len(kat["sizes"])):
        for cfg in range(CONFIGS):
            tid = sc.add_texture(kat[f"tex{t}"], magFilter=cfg % 2, minFilter=cfg % 2, wrapS=cfg // 6, wrapT=(cfg // 2) % 3)
            assert sc.add_material(pbrBaseColorTexture=tid) == tid == t * CONFIGS + cfg
    add_quad(sc, 0)
    return sc.finalize(capi.pack_vertices)


def ints(*cols):
    return [np.asarray(c).astype(np.int32).view(np.float32) for c in cols]


def rows(*cols):
    """probe rows from columns (float32 columns as they are; make integer columns with ints())"""
    n = max(np.size(c) for c in cols)
    r = np.zeros((n, IN), np.float32)
    for k, c in enumerate(cols):
        r.view(np.uint32)[:, k] = np.broadcast_to(np.asarray(c, np.float32), (n,)).view(np.uint32)
    return r


def fixture_rows(kat, slot=-1):
    tid = kat["row_tex"].astype(np.int32) * CONFIGS + kat["row_cfg"]
    return rows(*ints(tid, np.full(len(tid), slot)), kat["row_u"], kat["row_v"])


def probe(fn, handle, kind, r, fill=np.nan):
    """the rows through one call; returns (n, OUT) float32 (rows the probe refuses keep `fill`)"""
    r = np.ascontiguousarray(r, np.float32)
    out = np.full((len(r), OUT), fill, np.float32)
    rc = fn(handle, kind, len(r), r.ctypes.data, r.shape[1], out.ctypes.data, OUT)
    assert rc == 0, f"texture probe {kind} failed with {rc}"
    return out


class HostScene:
    """the product's records, lines, maps and pool for a scene (tests/cpp/trace_host.cpp th_create_scene) under one PT_TUNE setting"""

    def __init__(self, scene, tune=None, expect_error=False):
        from tests import host_harness
        L = self.L = host_harness.lib()
        d, self.keep = scene.desc()
        err = C.create_string_buffer(256)
        with tuned(tune):
            self.h = L.th_create_scene(C.byref(d), err, 256, host_harness.MERGE_SINGLES)
        self.error = err.value.decode()
        if expect_error:
            return
        assert self.h, self.error
        counts = np.zeros(4, np.uint64)
        L.th_texture_records(self.h, counts.ctypes.data, None, None, None, None, None)
        self.tex_recs = np.zeros((int(counts[0]), 8), np.int32)      # offset w h mag wrapS wrapT pot tiled
        self.mat_lines = np.zeros((int(counts[1]), 8, 4), np.uint32)
        self.alpha_mats = np.zeros((int(counts[1]), 20), np.uint32)  # AlphaMat, 80 bytes
        self.alpha_maps = np.zeros(int(counts[2]), np.uint32)
        self.texels = np.zeros(int(counts[3]), np.uint32)
        L.th_texture_records(self.h, counts.ctypes.data, self.tex_recs.ctypes.data, self.mat_lines.ctypes.data, self.alpha_mats.ctypes.data, self.alpha_maps.ctypes.data, self.texels.ctypes.data)

    def probe(self, kind, r, fill=np.nan):
        return probe(self.L.th_texture_probe, self.h, kind, r, fill)

    def set_env(self, img):
        img = np.ascontiguousarray(img, np.float32)
        integral = C.c_float()
        self.L.th_set_env(self.h, img.ctypes.data, img.shape[1], img.shape[0], C.byref(integral))
        self.env_keep = img

    def close(self):
        if self.h:
            self.L.th_destroy(C.c_void_p(self.h))
            self.h = None


def same_bits(a, b):
    """NaN in the same places, every other value equal as bits; returns the number of differing values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero(an != bn) + np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~an & ~bn))

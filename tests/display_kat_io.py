"""Reads tests/golden/display_kat.npz (minted by tests/golden/gen_display_kat.py) and runs the CPU legs of the display pass on it -- test infrastructure.

The fixture's model is imported only for what the tests need of it a second time: the error measure, and shade() with a forced local-exposure exit (the
candidates a leg's fragColor is matched against).  Nothing here feeds the legs anything but the fixture's inputs.
"""
import ctypes as C
import os
import sys

import numpy as np

from tests import orc, ref
from vk_raytrace_amd import host_device as hd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import gen_display_kat as gen  # noqa: E402

NO_BREAK = gen.NO_BREAK
U = 2.0 ** -23


def load():
    with np.load(os.path.join(GOLDEN, "display_kat.npz")) as z:
        return {k: z[k] for k in z.files}


class Image:
    """one input of the fixture: the render (h, w, 4), the viewport (W, H) it is shown in, zoom = num / den"""

    def __init__(self, kat, name):
        k = list(kat["image_names"]).index(name)
        w, h, x0, y0, W, H, num, den = (int(v) for v in kat["image_geometry"][k])
        self.name, self.w, self.h, self.W, self.H, self.num, self.den = name, w, h, W, H, num, den
        self.render = np.ascontiguousarray(kat["master"][y0:y0 + h, x0:x0 + w])
        self.zoom = float(np.float32(num) / np.float32(den))
        self.levels = int(kat[f"chain_{name}_levels"])

    def padded(self):
        out = np.zeros((self.H, self.W, 4), np.float32)
        out[:self.h, :self.w] = self.render
        return out

    def model_chain(self, kat):
        """the model's chain, float64 rounded to float32; level 0 is the padded input itself"""
        return [self.padded()] + [kat[f"chain_{self.name}_{lod}"] for lod in range(1, self.levels)]


def images(kat):
    return [Image(kat, n) for n in kat["image_names"]]


def tonemapper(kat, case, zoom=1.0):
    """hd.Tonemapper of a case of the fixture, and the model's dict of it"""
    v = dict(zip(kat["tm_fields"], kat[f"tm_{case}"]))
    tm = hd.Tonemapper(brightness=v["brightness"], contrast=v["contrast"], saturation=v["saturation"], vignette=v["vignette"], avgLum=v["avgLum"], zoom=zoom,
                       renderingRatio=(v["renderingRatio0"], v["renderingRatio1"]), autoExposure=int(v["autoExposure"]), Ywhite=v["Ywhite"], key=v["key"], dither=int(v["dither"]))
    d = {k: (int(x) if k in ("autoExposure", "dither") else float(x)) for k, x in v.items()}
    d["zoom"] = float(np.float32(zoom))
    return tm, d


class Run:
    def __init__(self, kat, k, prefix="run"):
        self.k, self.key = k, f"{prefix}{k}"
        if prefix == "run":
            self.image = Image(kat, str(kat["run_image"][k]))
            self.case = str(kat["run_case"][k])
            self.label = f"{self.image.name} / {self.case}"
        else:  # an edge run: a 3 x 2 image of its own, shown 1:1
            self.image = Image.__new__(Image)
            im = self.image
            im.name, im.w, im.h, im.W, im.H, im.num, im.den, im.zoom = str(kat["edge_names"][k]), 3, 2, 3, 2, 1, 1, 1.0
            im.render = np.ascontiguousarray(kat[f"edge{k}_in"])
            self.case = str(kat["edge_case"][k])
            self.label = im.name
        self.tm, self.tmd = tonemapper(kat, self.case, self.image.zoom)
        self.frag, self.code, self.kept, self.round_only = (kat[f"{self.key}_{n}"] for n in ("frag", "code", "kept", "round_only"))
        self.exit = kat[f"{self.key}_exit"] if f"{self.key}_exit" in kat else None
        self.local = self.tmd["autoExposure"] == 3


def runs(kat):
    return [Run(kat, k) for k in range(len(kat["run_image"]))]


def edges(kat):
    return [Run(kat, k, "edge") for k in range(len(kat["edge_names"]))]


# ---- the legs ---------------------------------------------------------------------------------------------------------------------------------------------
def orc_tonemap(run):
    """(fragColor floats, RGBA8) of the oracle's display pass on a run"""
    im = run.image
    L = orc.lib()
    L.orc_tonemap_zoom.argtypes = [C.POINTER(hd.Tonemapper), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    f, c = np.zeros((im.H, im.W, 4), np.float32), np.zeros((im.H, im.W, 4), np.uint8)
    assert L.orc_tonemap_zoom(C.byref(run.tm), im.render.ctypes.data, im.w, im.h, im.W, im.H, c.ctypes.data, f.ctypes.data) == 0
    return f, c


def ref_tonemap(run):
    """fragColor floats of the compiled post.frag on the padded viewport image"""
    im = run.image
    f, big = np.zeros((im.H, im.W, 4), np.float32), im.padded()
    ref.lib().ref_tonemap(C.byref(run.tm), big.ctypes.data, im.W, im.H, f.ctypes.data)
    return f


def quantise(frag):
    """the project's float -> UNORM8 store (oracle/pt_oracle.cpp unorm8) on an array of floats"""
    frag = np.ascontiguousarray(frag, np.float32)
    out = np.zeros(frag.shape, np.uint8)
    L = orc.lib()
    L.orc_unorm8.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p]
    assert L.orc_unorm8(frag.size, frag.ctypes.data, out.ctypes.data) == 0
    return out


def chain_of(side, level0):
    """every level of orc_mip_chain / ref_mip_chain on an image"""
    L, fn = (orc.lib(), "orc_mip_chain") if side == "orc" else (ref.lib(), "ref_mip_chain")
    f = getattr(L, fn)
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    level0 = np.ascontiguousarray(level0, np.float32)
    H, W = level0.shape[:2]
    n = f(level0.ctypes.data, W, H, -1, None, None, None)
    out = []
    for lod in range(n):
        w, h = C.c_int(), C.c_int()
        f(level0.ctypes.data, W, H, lod, None, C.byref(w), C.byref(h))
        lv = np.zeros((h.value, w.value, 4), np.float32)
        f(level0.ctypes.data, W, H, lod, lv.ctypes.data, C.byref(w), C.byref(h))
        out.append(lv)
    return out


# ---- what the tests assert ----------------------------------------------------------------------------------------------------------------------------------
def chain_bounds(model_chain):
    """per level and channel: the bound on |leg - model| (tests/test_display_model.py derives it).  One blit adds (sw + sh + 4) 2^-23 max|source texel|
    and inherits the source level's bound (the filter is a convex combination); the fixture stores the model rounded to float32: + 2^-24 |texel|."""
    bounds = [np.zeros(4)]
    for lod in range(1, len(model_chain)):
        sh, sw = model_chain[lod - 1].shape[:2]
        bounds.append(bounds[-1] + (sw + sh + 4) * U * np.abs(model_chain[lod - 1].astype(np.float64)).reshape(-1, 4).max(0))
    return bounds


def check_chain(got, model_chain, what):
    assert len(got) == len(model_chain), f"{what}: {len(got)} levels, the model has {len(model_chain)}"
    worst = 0.0
    for lod, (g, m, b) in enumerate(zip(got, model_chain, chain_bounds(model_chain))):
        assert g.shape == m.shape, f"{what}: level {lod} is {g.shape[1]} x {g.shape[0]}, the model's {m.shape[1]} x {m.shape[0]}"
        err = np.abs(g.astype(np.float64) - m.astype(np.float64))
        lim = b[None, None, :] + 0.5 * U * np.abs(m.astype(np.float64))
        assert (err <= lim).all(), f"{what}: level {lod} off by {err.max():.3g} (bound {lim.max():.3g}) at {np.unravel_index(np.argmax(err - lim), err.shape)}"
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()) if lod else 0.0)
    return worst


def check_codes(codes, run, what):
    """the model's codes on kept pixels, within 1 of them on the pixels dropped for the final rounding only"""
    k, r = run.kept, run.round_only
    bad = (codes[k] != run.code[k]).any(-1)
    assert not bad.any(), f"{what}, {run.label}: {int(bad.sum())} of {int(k.sum())} kept pixels differ from the model, first {codes[k][bad][0]} for {run.code[k][bad][0]}"
    d = np.abs(codes[r].astype(np.int32) - run.code[r].astype(np.int32))
    assert (d <= 1).all(), f"{what}, {run.label}: a pixel dropped for the final rounding is off by {int(d.max())} codes"


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    va, vb = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
    both_nan = np.isnan(a) & np.isnan(b) if a.dtype == np.float32 else np.zeros(a.shape, bool)  # a NaN is a NaN: its payload is not part of the contract
    bad = (va != vb) & ~both_nan
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} against {b[bad][0]!r}"


def recovered_exit_errors(frag, run, model_chain):
    """(8, H, W): the measure of a leg's fragColor against the model's fragColor had toneLocalExposure left at break i = 0..6 / not at all"""
    chain = [lv.astype(np.float64) for lv in model_chain]
    H, W = chain[0].shape[:2]
    return np.stack([gen.measure(frag, gen.shade(chain, run.tmd, forced_exit=np.full((H, W), e))[0]) for e in range(8)])

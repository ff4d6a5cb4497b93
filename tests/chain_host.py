"""The host build of the chained guide pass (tests/cpp/chain_host.cpp: vk_raytrace_amd/csrc/pt_chain.h compiled by g++) and its
Python side.  The library is one of host_harness.build_library's, cached under tests/cpp/_build/.  It works on the scene handle a
host_harness.TracedScene holds, with the camera guides_host.set_camera gave it.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import host_harness as hh
from vk_raytrace_amd import host_device as hd

_P = C.c_void_p
_CH = C.POINTER(hd.GuideChain)
SIGNATURES = [
    ("ch_constants", C.c_int, [_CH, C.c_char_p, C.c_int]),
    ("ch_need_plane", C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    ("ch_chain", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _CH, C.c_uint32, C.c_float, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("ch_links", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _CH, C.c_float, C.c_int, _P, _P, _P, C.POINTER(C.c_uint32)]),
]
_host = hh.StageLibrary("libchainhost", "chain_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib

LINK_WORDS, LINK_SLOTS = 28, 9
END, MIRROR, GLASS, THIN, TIR = range(5)                       # a link record's class
END_SURFACE, END_MISS, END_LIMIT, END_DIR = range(4)           # the link plane's end code (word >> 8); word & 255: the links followed
# a link record as ch_links writes it
link_dtype = np.dtype([("org", np.float32, 3), ("dir", np.float32, 3), ("seed", np.uint32), ("t", np.float32), ("instance", np.uint32), ("primitive", np.uint32),
                       ("ffnormal", np.float32, 3), ("position", np.float32, 3), ("roughness", np.float32), ("metallic", np.float32), ("transmission", np.float32),
                       ("eta", np.float32), ("thin", np.uint32), ("albedo", np.float32, 3), ("cls", np.uint32), ("u", np.float32), ("v", np.float32), ("ref", np.uint32)])
assert link_dtype.itemsize == 4 * LINK_WORDS


def params(max_links=8, max_roughness=0.05, min_metallic=0.9, min_transmission=0.9, flags=0):
    return hd.GuideChain(maxLinks=max_links, maxRoughness=max_roughness, minMetallic=min_metallic, minTransmission=min_transmission, flags=flags)


def constants(p, L=None):
    """(status, reason) of chain_constants"""
    why = C.create_string_buffer(160)
    rc = (L or lib()).ch_constants(None if p is None else C.byref(p), why, 160)
    return rc, why.value.decode()


def need_plane(have, L=None):
    why = C.create_string_buffer(160)
    rc = (L or lib()).ch_need_plane(int(have), why, 160)
    return rc, why.value.decode()


def chain(traced, two, width, height, p, planes=7, miss_depth=1.0e30, into=None, L=None, overflow_ok=False):
    """ch_chain: (planes, link plane) -- three (H, W, 4) float32 images and an (H, W) uint32 one -- of the scene `traced` holds for the camera
    guides_host.set_camera gave it.  A plane outside `planes` is not written: it keeps what `into` holds, or comes back as None.  overflow_ok: the
    number of traversal-stack overflows is returned as a third value instead of being asserted to be 0"""
    out = [None] * 3
    for j in range(3):
        if into is not None and into[j] is not None:
            out[j] = into[j]
            assert out[j].dtype == np.float32 and out[j].shape == (height, width, 4) and out[j].flags.c_contiguous
        elif planes & (1 << j):
            out[j] = np.zeros((height, width, 4), np.float32)
    links = np.zeros((height, width), np.uint32)
    over = C.c_uint32()
    rc = (L or lib()).ch_chain(traced.h, int(two), width, height, C.byref(p), planes, miss_depth, *[None if q is None else q.ctypes.data for q in out], links.ctypes.data, C.byref(over))
    assert rc == 0, rc
    if overflow_ok:
        return tuple(out), links, over.value
    assert over.value == 0, "traversal stack overflow"
    return tuple(out), links


def links(traced, two, width, height, p, pixels=None, miss_depth=1.0e30, L=None):
    """ch_links: (records (n, LINK_SLOTS) of link_dtype, counts (n,)) for the pixels (row-major indices; None: every pixel)"""
    pixels = np.arange(width * height, dtype=np.uint32) if pixels is None else np.ascontiguousarray(pixels, np.uint32)
    rec = np.zeros((len(pixels), LINK_SLOTS), link_dtype)
    counts = np.zeros(len(pixels), np.uint32)
    over = C.c_uint32()
    rc = (L or lib()).ch_links(traced.h, int(two), width, height, C.byref(p), miss_depth, len(pixels), pixels.ctypes.data, rec.ctypes.data, counts.ctypes.data, C.byref(over))
    assert rc == 0 and over.value == 0, (rc, over.value)
    return rec, counts

"""The display pass on the device -- k_pad_corner, k_blit_linear, k_tonemap (csrc/pt_render.hip) behind pt_tonemap / pt_tonemap_zoom / pt_tonemap_begin
(csrc/pt_capi.hip) -- held to the independent model of tests/golden/gen_display_kat.py AND to the oracle, through the public ABI.

pt_write_accum takes an arbitrary image and needs only pt_resize: no scene, no rendered frame.  Per input of the fixture: pt_resize, pt_write_accum(image),
then every run of that input through pt_tonemap (viewport == image) or pt_tonemap_zoom (de-scaled), and once per input through pt_tonemap_begin /
pt_tonemap_end.  The RGBA8 image must equal the model's codes on kept pixels, be within 1 code on the pixels the model dropped for the final rounding only,
and be byte-identical to the oracle's on EVERY pixel, edge runs (NaN, infinities, black, 3e38) included.
The chain is not visible in the RGBA8 image except through the exposure, so pt_debug_display_level copies one level of the offscreen image back; it runs the
very function pt_tonemap_zoom builds the chain with (pt_capi.hip display_chain).  Every device level: within the bound tests/test_display_model.py derives of
the model, and bit-identical to orc_mip_chain -- at the de-scaled sizes too, which is where the zero padding (alpha included) shows.
One context serves every size and case.  Launch blocks are 16 x 16 (pt_launch_tonemap / _blit_linear / _pad_corner): 33 x 17 crosses one in both directions.

The plumbing the injection relies on sits here as well: pt_write_accum -> pt_read_accum returns arbitrary bit patterns unchanged (edge tiles of k_retile /
k_untile: sizes that are no multiple of the 32 x 32 tile), a (1, 2) shard returns its own tiles and zero elsewhere, a viewport smaller than the image is an
error for both pt_tonemap_zoom and pt_tonemap_begin.
"""
import ctypes as C

import numpy as np
import pytest

from tests import display_kat_io as io
from vk_raytrace_amd import capi, host_device as hd

pytestmark = pytest.mark.gpu

IMAGE_NAMES = [i[0] for i in io.gen.IMAGES]


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def dev():
    from vk_raytrace_amd.renderer import HipRenderer
    r = HipRenderer()
    r.setup(0)
    yield r
    r.destroy()


def show(r, run):
    im = run.image
    return r.tonemap(run.tm) if (im.W, im.H) == (im.w, im.h) else r.tonemap(run.tm, display_size=(im.W, im.H))


def check_run(r, run):
    got = show(r, run)
    io.check_codes(got, run, "device")
    io.same_bits(got, io.orc_tonemap(run)[1], f"device against the oracle, {run.label}")
    return got


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_rgba8_equals_the_model_and_the_oracle(kat, dev, name):
    mine = [run for run in io.runs(kat) if run.image.name == name]
    assert mine
    im = mine[0].image
    dev.create((im.w, im.h))
    dev.write_accum(im.render)
    shown = [check_run(dev, run) for run in mine]
    # the pipelined entry: the same images, begun back to back and collected in order
    for run in mine[:capi.PT_DISPLAY_RING]:
        dev.tonemap_begin(run.tm, display_size=(im.W, im.H))
    for run, want in zip(mine[:capi.PT_DISPLAY_RING], shown):
        io.same_bits(dev.tonemap_end(), want, f"pt_tonemap_begin / pt_tonemap_end, {run.label}")


def test_edge_runs(kat, dev):
    dev.create((3, 2))
    n = 0
    for run in io.edges(kat):
        dev.write_accum(run.image.render)
        got = check_run(dev, run)
        if "no exposure" not in run.label and any(t in run.label for t in ("NaN", "Inf", "all-black")):
            assert (got[..., :3] == 0).all(), run.label  # the exposure is NaN (or 0) for every pixel: all colour codes are 0
            n += 1
    assert n == 8


def device_chain(r, W, H):
    L, out = capi.lib(), []
    n = L.pt_debug_display_level(r._ctx, W, H, -1, None, None, None)
    r._check(min(n, 0))
    for lod in range(n):
        w, h = C.c_int(), C.c_int()
        r._check(min(L.pt_debug_display_level(r._ctx, W, H, lod, None, C.byref(w), C.byref(h)), 0))
        lv = np.zeros((h.value, w.value, 4), np.float32)
        assert L.pt_debug_display_level(r._ctx, W, H, lod, lv.ctypes.data, C.byref(w), C.byref(h)) == n
        out.append(lv)
    return out


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_every_device_level_is_the_models_and_the_oracles(kat, dev, name):
    im = io.Image(kat, name)
    dev.create((im.w, im.h))
    dev.write_accum(im.render)
    got = device_chain(dev, im.W, im.H)
    io.same_bits(got[0], im.padded(), f"{name}: level 0 is the image in the corner of a zeroed viewport")
    io.check_chain(got, im.model_chain(kat), f"device, {name}")
    for lod, (a, b) in enumerate(zip(got, io.chain_of("orc", im.padded()))):
        io.same_bits(a, b, f"device against orc_mip_chain, {name} level {lod}")


def patterns(w, h, seed):
    """arbitrary bit patterns: random words, with denormals, both zeros, infinities and NaNs of either sign with payloads placed by hand"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000001, 0x807FFFFF, 0x80000000, 0x00000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00800000], np.uint32)
    flat = bits.reshape(-1)
    flat[rng.permutation(flat.size)[:min(flat.size, 3 * len(special))]] = np.resize(special, min(flat.size, 3 * len(special)))
    return bits.view(np.float32)


@pytest.mark.parametrize("size", [(1, 1), (33, 31), (100, 37)])
def test_write_accum_then_read_accum_is_the_identity(dev, size):
    img = patterns(size[0], size[1], size[0])
    dev.create(size)
    dev.write_accum(img)
    got = dev.read_accum()
    assert np.array_equal(got.view(np.uint32), img.view(np.uint32))
    # and the display pass reads the same image: level 0 of its chain, bit for bit
    assert np.array_equal(device_chain(dev, size[0], size[1])[0].view(np.uint32), img.view(np.uint32))


def test_a_shard_returns_its_own_tiles_and_zero_elsewhere():
    from vk_raytrace_amd.renderer import HipRenderer
    w, h, T = 100, 37, 32
    img = patterns(w, h, 5)
    r = HipRenderer()
    r.setup(0)
    try:
        r.set_shard(1, 2)
        r.create((w, h))
        r.write_accum(img)
        got = r.read_accum()
    finally:
        r.destroy()
    yy, xx = np.mgrid[0:h, 0:w]
    own = ((xx // T + yy // T) % 2 == 1)[..., None]  # pt_resize: tile (tx, ty) belongs to rank (tx + ty) % nranks
    assert own.any() and not own.all()
    assert np.array_equal(got.view(np.uint32), np.where(own, img.view(np.uint32), 0))


def test_a_viewport_smaller_than_the_image_is_an_error(dev):
    dev.create((33, 17))
    dev.write_accum(np.ones((17, 33, 4), np.float32))
    tm = hd.default_tonemapper()
    out = np.zeros((17, 33, 4), np.uint8)
    L = capi.lib()
    for W, H in ((32, 17), (33, 16), (1, 1)):
        assert L.pt_tonemap_zoom(dev._ctx, C.byref(tm), W, H, out.ctypes.data) == capi.PT_ERR_INVALID
        assert L.pt_tonemap_begin(dev._ctx, C.byref(tm), W, H) == capi.PT_ERR_INVALID
        assert L.pt_debug_display_level(dev._ctx, W, H, 0, None, None, None) == capi.PT_ERR_INVALID
    assert L.pt_tonemap_pending(dev._ctx) == 0  # nothing was enqueued
    assert (dev.tonemap(tm)[..., 3] == 255).all()  # and the context still works

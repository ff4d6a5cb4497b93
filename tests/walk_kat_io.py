"""Shared by tests/test_walk_model.py and tests/test_walk_gpu.py: the fixture of tests/golden/gen_walk_kat.py, the scene it describes, and the rules by which a
leg's answers are held to the model.  A leg hands over plain arrays (or pt_RayHit records); every check returns the mask of kept rays it compared, so that the
census can be asserted over rays a leg actually answered.

What must agree on the kept rays: committed instance, primitive and instanceCustomIndex (a miss is a miss), the shadow verdict, the seed afterwards and the number
of draws where a leg reports it -- bit for bit; t, u, v within B(t), B(u), B(v) of the float64 values, on exact rows and zero-draw rays bit for bit.  No allowance
for differing rays: the kept mask is what removes ill-conditioned ones."""
import functools
import importlib.util
import os

import numpy as np

from tests import surface_kat_io
from vk_raytrace_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HIT = capi.PT_RAY_HIT
NONE = 0xFFFFFFFF
F_EXACT, F_ZERO = 4, 5
KEYS = 16


@functools.lru_cache(None)
def generator():
    spec = importlib.util.spec_from_file_location("gen_walk_kat", os.path.join(GOLDEN, "gen_walk_kat.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def load(path=None):
    with np.load(path or os.path.join(GOLDEN, "walk_kat.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_scene(kat, opaque=False):
    """the fixture's arrays as a Scene (tests/surface_kat_io.py: the packed vertices word for word, one prim-mesh record per piece, the nodes with their
    matrices).  opaque: a copy with alphaMode 0 on every material -- the any-hit-off form for legs that have no switch for it"""
    sc = surface_kat_io.fixture_scene(kat)
    if opaque:
        for m in sc.materials:
            m["alphaMode"] = 0
    return sc


def check_scene_words(kat, sc):
    """the scene a leg is given holds the fixture's words: packed vertices, indices, prim-mesh records, matrices, materials, texels"""
    d, keep = sc.desc()
    verts, idx, pm, nd, mats, _, tex = keep
    assert np.array_equal(verts["position"].view(np.uint32), kat["position"].view(np.uint32)) and np.array_equal(verts["texcoord"].view(np.uint32), kat["texcoord"].view(np.uint32))
    assert np.array_equal(verts["normal"], kat["normal_code"]) and np.array_equal(verts["tangent"], kat["tangent_code"]) and np.array_equal(verts["color"], kat["color_code"])
    assert np.array_equal(idx, kat["indices"]) and idx.dtype == np.uint32
    assert np.array_equal(np.array(pm.tolist(), np.int32), kat["records"])
    assert np.array_equal(nd["primMesh"], kat["node_record"])
    got = nd["worldMatrix"].reshape(-1, 4, 4).transpose(0, 2, 1)                     # column-major words
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), kat["node_matrix"].view(np.uint32))
    assert mats.tobytes() == kat["materials"].tobytes()
    assert d.numTextures == len(kat["tex_sampler"])
    for t, (mag, ws, wt) in enumerate(kat["tex_sampler"]):
        assert np.array_equal(sc.textures[t].rgba8, kat[f"tex{t}"]) and (tex[t].magFilter, tex[t].wrapS, tex[t].wrapT) == (mag, ws, wt), t
    return keep


def rays(kat, n=None):
    from tests.test_query_host import make_rays
    n = len(kat["ray_seed"]) if n is None else n
    return make_rays(kat["ray_origin"][:n], kat["ray_direction"][:n], tmax=kat["ray_tmax"][:n], seeds=kat["ray_seed"][:n])


def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fail(what, bad, kat, detail=""):
    r = np.nonzero(bad)[0]
    fam = kat["family_names"][kat["ray_family"][r[:8]]]
    return f"{what}: {len(r)} kept rays differ from the model, first {r[:8]} (families {list(fam)}) {detail}"


def check_closest(kat, what, world, tuv, seed, draws=None, opaque=False, ids=None):
    """T5.  world: (n,) world triangle index, NONE or -1 for a miss; tuv (n, 3) float32; seed (n,) afterwards; draws (n,) or None; opaque: the any-hit-off form
    (nearest key, the seed untouched); ids: (instanceID, primitiveID, instanceCustomIndex) where the leg reports them"""
    n = len(world)
    kept = kat["kept"][:n]
    want_w = (kat["opaque_world"] if opaque else kat["closest_world"])[:n].astype(np.int64)
    want_tuv, bound = (kat["opaque_tuv"] if opaque else kat["closest_tuv"])[:n], (kat["opaque_bound"] if opaque else kat["closest_bound"])[:n]
    want_seed = kat["ray_seed"][:n] if opaque else kat["closest_seed"][:n]
    w = np.asarray(world).astype(np.int64)
    w[w == NONE] = -1
    bad = kept & (w != want_w)
    assert not bad.any(), _fail(what + " committed triangle", bad, kat, f"got {w[bad][:8]} want {want_w[bad][:8]}")
    bad = kept & (np.asarray(seed, np.uint32) != want_seed)
    assert not bad.any(), _fail(what + " seed afterwards", bad, kat)
    if draws is not None:
        bad = kept & (np.asarray(draws).astype(np.int64) != (0 if opaque else kat["closest_draws"][:n]))
        assert not bad.any(), _fail(what + " number of draws", bad, kat)
    hit = kept & (want_w >= 0)
    got = np.asarray(tuv, np.float32).astype(np.float64)
    err = np.abs(got - want_tuv)
    bad = hit & (err > bound).any(1)
    assert not bad.any(), _fail(what + " t, u, v outside B(t), B(u), B(v)", bad, kat, f"worst {np.max(err[hit] / np.maximum(bound[hit], 1e-300)):.3g} of the bound")
    exact = hit & (kat["ray_family"][:n] >= F_EXACT)
    bad = exact & (_f32_bits(tuv) != _f32_bits(want_tuv)).any(1)
    assert not bad.any(), _fail(what + " t, u, v bit for bit on exact rows", bad, kat)
    if ids is not None:
        inst, prim, custom = (np.asarray(x).astype(np.int64) for x in ids)
        k = np.maximum(want_w, 0)
        wi, wp, wc = (np.where(want_w >= 0, kat[name][k].astype(np.int64), np.int64(miss)) for name, miss in (("world_inst", NONE), ("world_prim", -1), ("world_pm", -1)))
        bad = kept & ((inst != wi) | (prim != wp) | (custom != wc))
        assert not bad.any(), _fail(what + " instance, primitive, instanceCustomIndex", bad, kat)
    print(f"{what}: {int(kept.sum())} kept rays, {int(hit.sum())} hits, worst t/u/v error {np.max(err[hit] / np.maximum(bound[hit], 1e-300)) if hit.any() else 0:.3f} of its bound")
    return kept


def check_shadow(kat, what, in_shadow, seed, variant, draws=None, opaque=False):
    """T6 on the rays' own tmax.  variant: capi.PT_VARIANT_RAYQUERY (the seed advanced) or PT_VARIANT_RTX (untouched)"""
    n = len(in_shadow)
    kept = kat["kept"][:n]
    want = (kat["opaque_shadow"] if opaque else kat["shadow_hit"])[:n]
    want_seed = kat["ray_seed"][:n] if opaque else (kat["shadow_seed_rtx"] if variant == capi.PT_VARIANT_RTX else kat["shadow_seed"])[:n]
    bad = kept & (np.asarray(in_shadow).astype(bool) != want)
    assert not bad.any(), _fail(what + " verdict", bad, kat)
    bad = kept & (np.asarray(seed, np.uint32) != want_seed)
    assert not bad.any(), _fail(what + " seed afterwards", bad, kat)
    if draws is not None:
        bad = kept & (np.asarray(draws).astype(np.int64) != (0 if opaque else kat["shadow_draws"][:n]))
        assert not bad.any(), _fail(what + " number of draws", bad, kat)
    return kept


def check_candidates(kat, what, world, t):
    """T4: the first 16 keys (t, world index) inside (0, tmax), before alpha.  world (n, 16), NONE or -1 where the list has ended; t (n, 16) float32"""
    n = len(world)
    kept = kat["kept"][:n]
    lim = kat["ray_tmax"][:n].astype(np.float64)[:, None]
    want_w, want_t = kat["key_world"][:n].astype(np.int64).copy(), kat["key_t"][:n]
    want_w[~((want_w >= 0) & (want_t < lim))] = -1
    w = np.asarray(world).astype(np.int64)
    w[w == NONE] = -1
    bad = kept & (w != want_w).any(1)
    assert not bad.any(), _fail(what + " key list", bad, kat)
    on = kept[:, None] & (want_w >= 0)
    got = np.asarray(t, np.float32)
    bad = (on & (np.abs(got.astype(np.float64) - want_t) > kat["key_bt"][:n])).any(1)
    assert not bad.any(), _fail(what + " key t outside B(t)", bad, kat)
    exact = on & (kat["ray_family"][:n] >= F_EXACT)[:, None]
    bad = (exact & (_f32_bits(got) != _f32_bits(want_t))).any(1)
    assert not bad.any(), _fail(what + " key t bit for bit on exact rows", bad, kat)
    return kept


def records_closest(kat, what, recs, opaque=False):
    """pt_RayHit records of a CLOSEST query against the model; the world triangle is named by the record's own (instanceID, primitiveID)"""
    hit = (recs["status"] & HIT) != 0
    assert ((recs["status"] & ~np.uint32(HIT)) == 0).all(), "no ray of the fixture is invalid"
    w = world_of(kat, recs)
    assert ((w >= 0) == hit).all()
    return check_closest(kat, what, w, np.stack([recs["t"], recs["u"], recs["v"]], 1), recs["seed"], opaque=opaque,
                         ids=(recs["instanceID"], recs["primitiveID"], recs["instanceCustomIndex"]))


def records_shadow(kat, what, recs, variant, opaque=False):
    assert (recs["instanceID"] == NONE).all() and (recs["t"] == 0).all() and (recs["primitiveID"] == -1).all()   # OCCLUDED fills no hit field
    return check_shadow(kat, what, (recs["status"] & HIT) != 0, recs["seed"], variant, opaque=opaque)


def records_candidates(kat, what, recs):
    assert (recs["seed"] == kat["ray_seed"][:len(recs), None]).all()
    w = world_of(kat, recs)
    assert ((w >= 0) == ((recs["status"] & HIT) != 0)).all()
    return check_candidates(kat, what, w, recs["t"])


def world_of(kat, recs):
    """(instanceID, primitiveID) -> world triangle index by the fixture's own table, -1 on a miss"""
    first = np.zeros(len(kat["node_record"]) + 1, np.int64)
    np.add.at(first, kat["world_inst"].astype(np.int64) + 1, 1)
    first = np.cumsum(first)
    inst = recs["instanceID"].astype(np.int64)
    miss = recs["instanceID"] == NONE
    w = first[np.where(miss, 0, inst)] + recs["primitiveID"]
    return np.where(miss, -1, w)


def census(kat, answered, small=4, large=50):
    """kept rays per tag among the rays a leg answered (a check's return value) -> {tag: count}; asserts the caps of the generator"""
    names = [str(x) for x in kat["tag_names"]]
    n = len(answered)
    counts = {name: int((((kat["tags"][:n] >> np.uint64(k)) & np.uint64(1)) != 0)[answered].sum()) for k, name in enumerate(names)}
    short = [f"{name}: {c}" for name, c in counts.items() if c < (small if (name.startswith("0.0 on") or name.startswith("exact row")) else large)]
    assert not short, "classes with too few answered rays: " + "; ".join(short)
    return counts


def drops(kat):
    """dropped fraction per ray family"""
    return {str(name): 1.0 - kat["kept"][kat["ray_family"] == f].mean() for f, name in enumerate(kat["family_names"])}


# ---- the frames case: kernels the C ABI cannot seed --------------------------------------------------------------------------------------------------
CARD_COLOUR = (0.125, 0.875, 0.25)   # no other material of the fixture has it
CAMERA = dict(eye=(0.0, 1.0, 30.0), center=(0.0, 1.0, 0.0), fov=40.0)
FRAME_SIZE = 64


def with_card(kat):
    """the fixture's arrays plus one screen-filling BLEND card of factor 0 in front of the camera: the first candidate of every primary ray"""
    out = dict(kat)
    nv, ni = len(kat["position"]), len(kat["indices"])
    quad = np.array([(-20, -19, 24), (20, -19, 24), (20, 21, 24), (-20, 21, 24)], np.float32)
    out["position"] = np.concatenate([kat["position"], quad])
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    uv[:, 1] = ((uv[:, 1].view(np.uint32) & np.uint32(0xFFFFFFFE)) | np.uint32(1)).view(np.float32)
    out["texcoord"] = np.concatenate([kat["texcoord"], uv])
    for k in ("normal_code", "tangent_code", "color_code"):
        out[k] = np.concatenate([kat[k], np.repeat(kat[k][:1], 4)])
    out["indices"] = np.concatenate([kat["indices"], np.array([0, 1, 2, 0, 2, 3], np.uint32)])
    card = kat["materials"][1:2].copy()   # "zero": BLEND, factor 0, double-sided
    assert card["alphaMode"][0] == 2 and card["pbrBaseColorFactor"][0, 3] == 0 and card["doubleSided"][0] == 1
    card["pbrBaseColorFactor"][0, :3] = CARD_COLOUR
    out["materials"] = np.concatenate([kat["materials"], card])
    out["records"] = np.concatenate([kat["records"], np.array([(nv, 4, ni, 6, len(kat["materials"]))], np.int32)])
    out["node_record"] = np.concatenate([kat["node_record"], np.array([len(kat["records"])], np.int32)])
    out["node_matrix"] = np.concatenate([kat["node_matrix"], np.eye(4, dtype=np.float32)[None]])
    return out


def first_traversal_draw_is_zero(frame, size=FRAME_SIZE):
    """the pixels of frame `frame` (> 0, maxSamples 1, ray query) whose first traversal draw is exactly 0.0, from gen_kat.tea and gen_path_kat's restatement of
    samplePixel's draw order: seed = tea(W y + x, frame); two jitter draws (frame > 0), two lens draws, then ClosestHit -- the fifth draw"""
    generator()                          # (puts tests/golden on the path)
    from gen_kat import pcg_step, tea
    assert frame > 0
    s = tea(np.arange(size * size, dtype=np.uint64), np.full(size * size, frame, np.uint64))
    for _ in range(5):
        s, w = pcg_step(s)
    return np.nonzero((w >> np.uint32(9)) == 0)[0]


def first_zero_frame(size=FRAME_SIZE, limit=1 << 16):
    """the first frame index upward from 1 that has such a pixel -> (frame, its pixels)"""
    for frame in range(1, limit):
        px = first_traversal_draw_is_zero(frame, size)
        if len(px):
            return frame, px
    raise AssertionError("no frame found")


def frames_config(kat, debug=0):
    """the fixture scene with the card at 64 x 64, maxDepth 2, maxSamples 1, under a small constant environment"""
    from tests.common import Config
    from vk_raytrace_amd.scene import Camera
    sc = surface_kat_io.fixture_scene(with_card(kat))
    sc.camera = Camera(**CAMERA)
    env = np.ones((2, 4, 4), np.float32)
    env[..., :3] = 0.5
    return Config(sc, env, FRAME_SIZE, FRAME_SIZE, depth=2, max_samples=1, debug=debug)


def card_pixels(img, frame):
    """pixels of a single-frame eBaseColor image rendered with frame index `frame` into a zeroed buffer (mix(0, colour, 1 / (frame + 1))) that show the card"""
    rgb = img[..., :3].astype(np.float64).reshape(-1, 3) * (frame + 1)
    return np.nonzero((np.abs(rgb - np.array(CARD_COLOUR)) < 1e-4).all(1))[0]

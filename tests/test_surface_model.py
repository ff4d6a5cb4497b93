"""Surface reconstruction and the material resolve held to an independent float64 model, per hit.

A hit is an instance, a primitive and two barycentrics; pt_surface.h surface_at_hit and resolve_material / resolve_material_at (with the lines of
shade_path around them) turn it into the Surface every BSDF call reads.  The legs:
    tests/golden/gen_surface_kat.py        the model: numpy, float64 and float32, written from the shader text (shares no code with any leg)
    ref_surface_probe  (oracle/_ref)       the reference's own GetShadeState + GetMaterialsAndTextures, compiled
    orc_surface_probe  (oracle/liborc.so)  the oracle's restatement
    th_surface_probe   (tests/cpp)         the product's headers, host build, on the product's own records / material lines / pool
    pt_debug_surface_probe                 the same function on the device, one row per lane
Row layout: vk_raytrace_amd/csrc/pt_probe.h.  Bound on kept rows: 4 x the error the compiled reference itself shows against float64, per output group
(tests/golden/surface_kat_tol.json, written by tests/golden/measure_surface_kat.py; never taken from the product); integer outputs exact; the legs equal
each other bit for bit on EVERY row, the named edge rows included (NaN in the same word counts as equal).

Questionable shader lines, followed as written: the handedness of vertex 0 alone scales the binormal (shade_state.glsl:114, h1 and h2 are computed and
dropped); the binormal is built from the normal BEFORE it is moved to the geometric side (:114 against :139); the normal-texture scale is applied after
the normalise, so a scaled normal is only renormalised by `normalize(TBN * v)` (gltf_material.glsl:122-124); max(0.001, x) = (0.001 < x ? x : 0.001) answers
0.001 for a NaN x, so anisotropy > 1 / 0.9 (sqrt of a negative number) ends as ax = ay = 0.001; a zero-area triangle has a NaN geometric normal, `dot <= 0` is
false for it and the normal is never flipped.

Proof that the check can fail (done once in a scratch copy).  The model broken one rule at a time (gen_surface_kat.BREAK), evaluated on the fixture's rows,
the UNCHANGED oracle held to it with the committed bound -- kept rows over the bound of 3682 / groups over the bound:
    h_vertex1               handedness from vertex 1                                3682   frame_bitangent bitangent (+ normal ffnormal tangent eta behind the normal maps)
    lsb_kept                uv LSB not cleared                                        26   albedo f0 alpha  (only the texture coordinates of 2^22 show it: near 1 the bit is an ulp)
    no_flip                 normal not moved to the geometric side                  1577   frame_normal normal ffnormal tangent bitangent eta
    ff_not_rederived        ffnormal kept from before normal mapping                 490   ffnormal tangent bitangent eta
    scale_before_unpack     normal scale applied to the texel, before 2 t - 1        244   normal ffnormal tangent bitangent eta
    scale_before_normalise  normalize(v * scale) for normalize(v) * scale              0   NOT a different function: TBN * v is linear and normalised afterwards, the factor
                                                                                           1 / |v * scale| against 1 / |v| drops out.  Listed because it was asked for; it cannot be caught.
    mr_rg                   r / g for g / b in the metallic-roughness texel          328   f0 metallic roughness ax ay
    pow24                   pow 2.4 for 2.2                                         1079   albedo emission f0
    clamp_dropped           max(roughness, 0.001) dropped                             97   roughness ax
    eta_inverted            eta choice inverted                                     3598   eta  (every row with ior != 1)
    aspect_no09             aspect without the 0.9                                   249   ax ay
    aniso_new_frame         anisotropic tangent from the frame after normal mapping  165   tangent bitangent
    ccr_from_r              clearcoat roughness from .r                              165   clearcoatRoughness
    uvt_colmajor            uvTransform read column-major                            588   uv and the twelve groups behind the textures
The product broken (pt_surface.h, host build only) -- the tests that fail, the other CPU tests of this file pass:
    h0 from v.b1.y (handedness of vertex 1)                       test_host_build_within_the_bound  test_legs_are_bit_identical
    the ffnormal line after normal mapping deleted                test_host_build_within_the_bound  test_legs_are_bit_identical
    clear_lsb returns y (uv LSB kept)                             test_host_build_within_the_bound  test_legs_are_bit_identical
    MAT_SIMPLE rebuild: m.normalTextureScale = 1.0f, not q1.w     test_host_build_within_the_bound  test_legs_are_bit_identical  test_line_path_equals_the_full_record
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import orc, ref, surface_kat_io as io, tex_kat_io
from vk_raytrace_amd import synth

FACTOR = 4.0   # the project's margin over the reference's own error (tests/test_float_kat.py)
AOV_MODES = {"base colour": 1, "normal": 2, "metallic": 3, "emissive": 4, "alpha": 5, "roughness": 6, "texcoord": 7,
             "tangent": 8}   # include/pt_types.h PT_DEBUG_*


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def gen():
    return io.generator()


@pytest.fixture(scope="module")
def tol():
    with open(os.path.join(io.GOLDEN, "surface_kat_tol.json")) as f:
        return json.load(f)["groups"]


@pytest.fixture(scope="module")
def scene(kat):
    return io.fixture_scene(kat)


@pytest.fixture(scope="module")
def oracle(scene):
    o = orc.Oracle()
    o.set_scene(scene)
    yield o
    o.close()


@pytest.fixture(scope="module")
def oracle_out(kat, oracle):
    out, rc = io.oracle_probe(oracle, io.STATE, io.probe_rows(kat))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def host(scene):
    h = io.HostScene(scene)
    yield h
    h.close()


@pytest.fixture(scope="module")
def host_out(kat, host):
    """(path 0, path 1)"""
    return tuple(host.probe(io.STATE, io.probe_rows(kat, path))[0] for path in (0, 1))


def over_the_bound(kat, tol, out):
    """(groups over the bound with their error, kept rows with a word over the bound or an integer word off)"""
    kept = kat["row_kept"]
    want, got = kat["want"].T[kept], io.values(out)[kept]
    bad_rows = np.zeros(int(kept.sum()), bool)
    groups = {}
    for name, (first, count) in zip(kat["group_names"], kat["group_words"]):
        w, g = want[:, first:first + count], got[:, first:first + count]
        with np.errstate(invalid="ignore"):
            e = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        e[np.isnan(e)] = np.inf
        over = e > FACTOR * tol[str(name)]
        if over.any():
            groups[str(name)] = float(e.max())
            bad_rows |= over.any(1)
    for w in io.INT_WORDS:
        off = got[:, w] != want[:, w]
        if off.any():
            groups[f"word {w}"] = float(off.sum())
            bad_rows |= off
    return groups, int(bad_rows.sum())


def check_leg(kat, tol, out, who):
    assert np.isfinite(out[kat["row_kept"]][:, :io.WORDS - 1]).all(), f"{who}: non-finite value on a kept row"
    groups, rows = over_the_bound(kat, tol, out)
    assert not groups, f"{who}: {rows} kept rows beyond {FACTOR:g} x the reference's own error: {groups}"


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_reproduces(gen, tmp_path):
    path = str(tmp_path / "again.npz")
    gen.main(path)
    with open(path, "rb") as a, open(os.path.join(io.GOLDEN, "surface_kat.npz"), "rb") as b:
        assert a.read() == b.read()
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(io.GOLDEN, f)) for f in os.listdir(io.GOLDEN) if f != "surface_kat.npz")


def test_fixture_reaches_every_case(kat, gen, tol):
    names = [str(n) for n in kat["material_names"]]
    mats, recs = kat["materials"], kat["records"]
    assert len(kat["indices"]) // 3 <= 64 and (recs[:, 4] == -1).sum() == 1 and (kat["normal_code"] == 0xFFFFFFFF).sum() == 1
    assert set(kat["node_class"].tolist()) == set(range(7)) and (np.bincount(kat["node_record"]) == 7).all()   # every record under every instance class
    det = np.linalg.det(kat["node_matrix"][:7, :3, :3].astype(np.float64))
    assert (det < 0).sum() == 2 and np.abs(kat["node_matrix"][1, :3, 3]).max() >= 1000.0
    tri = kat["indices"].reshape(-1, 3) + np.repeat(np.arange(5) * 12, 4)[:, None]
    hand = kat["texcoord"][:, 1].view(np.uint32)[tri] & 1
    assert (hand.min(1) != hand.max(1)).all() and len(set(hand[:, 0].tolist())) == 2   # corners differ in handedness; vertex 0 takes both values
    assert (kat["normal_code"][tri][:12, 0] != kat["normal_code"][tri][:12, 1]).all() and (kat["tangent_code"][tri][:12, 0] != kat["tangent_code"][tri][:12, 1]).all()
    # simplicity, from the rule in words: the plain material, the four texture flags, all four, and the materials that only change a field of the line
    simple = {n for n, s in zip(names, kat["simple"]) if s}
    assert simple == {"plain", "normal", "emissive", "metallic-roughness", "base colour", "all four", "normal scale 0.5", "normal scale 2", "roughness 0", "ior 1", "ior 2.4",
                      "roughness texture to the clamp"}
    for single in [f"uvTransform[{k}]" for k in range(8)] + ["transmission -0.0", "transmission texture", "anisotropy", "anisotropy direction", "attenuation colour 0",
                                                             "attenuation colour 1", "attenuation colour 2", "thickness", "attenuation distance", "clearcoat", "clearcoat roughness",
                                                             "clearcoat texture", "clearcoat roughness texture", "sheen", "unlit"]:
        m, d = mats[names.index(single)], mats[names.index("base colour" if single.startswith("uv") else "plain")]
        diff = [k for k in mats.dtype.names if not np.array_equal(np.atleast_1d(m[k]).view(np.uint32), np.atleast_1d(d[k]).view(np.uint32))]
        words = sum(int((np.atleast_1d(m[k]).view(np.uint32) != np.atleast_1d(d[k]).view(np.uint32)).sum()) for k in diff)
        assert len(diff) == 1 + single.startswith("uv") and words <= 2, (single, diff)   # ONE field breaks simplicity (the uvTransform materials also swap the texture)
    sizes = {(kat[f"tex{t}"].shape[1], kat[f"tex{t}"].shape[0], int(s[0])) for t, s in enumerate(kat["tex_sampler"])}
    assert sizes >= {(4, 4, 0), (4, 4, 1), (8, 4, 0), (8, 4, 1), (5, 3, 0), (5, 3, 1)}
    for t in range(len(kat["tex_sampler"])):
        assert kat[f"tex{t}"].min() == 0 and kat[f"tex{t}"].max() == 255
    # rows: every pair, every point kind and ray kind on every material and class; the kept mask is the model's, within the cap
    edge, kept = kat["row_edge"], kat["row_kept"]
    assert set(edge.tolist()) == set(range(7)) and not kept[edge != 0].any()
    assert 1.0 - kept[edge == 0].mean() <= 0.02
    pair = np.bincount(kat["row_inst"][kept], minlength=len(kat["node_record"]))
    node_mat = np.maximum(recs[kat["node_record"]][:, 4], 0)
    need = (kat["record_geometry"][kat["node_record"]] != 3) & (node_mat != names.index("anisotropy 1.25"))
    assert (kat["texcoord"][48:, 1] >= 2.0 ** 22).all()   # the far texture coordinates
    assert pair[need].min() >= 8
    mat_of_row = node_mat[kat["row_inst"]]
    assert len(set(zip(mat_of_row.tolist(), kat["row_kind"].tolist()))) == 3 * len(names)
    d = kat["row_dir"].astype(np.float64)
    wn = kat["want"].T[:, 3:6]
    graze = np.abs((d * wn).sum(1))[(kat["row_kind"] == 2) & (edge == 0)]
    assert graze.max() <= 1.001e-3 and graze.min() > 1e-4
    # the model again, here: the committed answers are the generator's
    want, kept2, edge2 = gen.evaluate(kat, {k[4:]: v for k, v in kat.items() if k.startswith("row_")})
    assert np.array_equal(want.T, kat["want"], equal_nan=True) and np.array_equal(kept2, kept) and np.array_equal(edge2, edge)
    assert set(tol) == {str(n) for n in kat["group_names"]} and max(tol.values()) <= 1e-3


# ---- CPU legs -----------------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_within_the_bound(kat, tol, oracle_out):
    check_leg(kat, tol, oracle_out, "oracle")


@pytest.mark.skipif(not ref.available(), reason="needs /root/reference (or a prebuilt oracle/_ref/libref.so)")
def test_reference_within_the_bound_and_equal_to_the_oracle(kat, tol, scene, oracle, oracle_out):
    r = ref.Reference(scene, synth.procedural_sky(16, 8), oracle=None)
    got, rc = io.reference_probe(r, io.STATE, io.probe_rows(kat))
    assert rc == 0
    check_leg(kat, tol, got, "compiled reference")
    groups, _ = over_the_bound(kat, {k: v / FACTOR for k, v in tol.items()}, got)   # the recorded error IS this leg's
    assert not groups, groups
    assert io.same_bits(got[:, :io.LINE_WORD], oracle_out[:, :io.LINE_WORD]) == 0, "oracle and compiled reference differ"
    assert io.reference_probe(r, io.SLOT, io.probe_rows(kat)[:4])[1] == io.NO_DATA and io.oracle_probe(oracle, io.SLOT, io.probe_rows(kat)[:4])[1] == io.NO_DATA


def test_host_build_within_the_bound(kat, tol, host_out):
    check_leg(kat, tol, host_out[0], "host build, path 0")
    check_leg(kat, tol, host_out[1], "host build, path 1")


def test_legs_are_bit_identical(kat, oracle_out, host_out):
    """every row, the named edge rows included"""
    a, b = host_out[0][:, :io.LINE_WORD], oracle_out[:, :io.LINE_WORD]
    an, bn = np.isnan(a), np.isnan(b)
    diff = (an != bn) | ((a.view(np.uint32) != b.view(np.uint32)) & ~an & ~bn)
    assert not diff.any(), f"host build and oracle differ on {int(diff.any(1).sum())} rows, words {np.nonzero(diff.any(0))[0].tolist()}, edge kinds {sorted(set(kat['row_edge'][diff.any(1)].tolist()))}"
    assert not np.isnan(a[:, :3]).any()   # every row was answered
    for k in range(1, 7):   # (every edge kind is among them, and the degenerate ones do produce what their name says)
        assert (kat["row_edge"] == k).sum() >= 4
    assert np.isnan(a[kat["row_edge"] == 1][:, 6:12]).any() and np.isnan(a[kat["row_edge"] == 6][:, 3:6]).any()   # no tangent left; a normal of 3.4e38
    assert (a[kat["row_edge"] == 5][:, 45:47] == np.float32(0.001)).all()   # sqrt of a negative number: max(0.001, NaN) is 0.001 as GLSL writes max


def test_line_path_equals_the_full_record(kat, host_out):
    p0, p1 = host_out
    assert io.same_bits(p0[:, :io.LINE_WORD], p1[:, :io.LINE_WORD]) == 0, "MAT_SIMPLE line path and full record differ"
    mat = p0[:, 67].view(np.uint32)
    assert np.array_equal(mat, np.maximum(kat["records"][kat["node_record"][kat["row_inst"]]][:, 4], 0))
    assert np.array_equal(p0[:, io.LINE_WORD].view(np.uint32) == 1, kat["simple"][mat]), "the line path is taken exactly for the materials the fixture marks simple"
    assert (p1[:, io.LINE_WORD].view(np.uint32) == 0).all() and kat["simple"].sum() >= 6 and (~kat["simple"]).sum() >= 25


def test_storage_settings_do_not_change_textured_rows(kat, scene, host_out):
    tex_fields = ("normalTexture", "emissiveTexture", "pbrMetallicRoughnessTexture", "pbrBaseColorTexture", "transmissionTexture", "clearcoatTexture", "clearcoatRoughnessTexture")
    textured = np.any([kat["materials"][k] > -1 for k in tex_fields], 0)
    sel = textured[host_out[0][:, 67].view(np.uint32)]
    assert sel.sum() > 1000
    r = io.probe_rows(kat, 0, sel)
    layouts = set()
    for tune in tex_kat_io.TUNES[1:]:
        h = io.HostScene(scene, tune)
        try:
            got, rc = h.probe(io.STATE, r)
            layouts.add(h.hs.mat_lines.tobytes())
        finally:
            h.close()
        assert rc == 0 and io.same_bits(got[:, :io.WORDS], host_out[0][sel][:, :io.WORDS]) == 0, f"PT_TUNE={tune}"
    assert len(layouts) == 3   # (the settings did change where the texels lie)


def refused_rows(kat):
    """rows outside the scene's counts: instance, primitive, path"""
    r = io.probe_rows(kat)[:6].copy()
    u = r.view(np.uint32)
    u[0, 0] = len(kat["node_record"])
    u[1, 0] = 0xFFFFFFFF
    u[2, 1] = 4
    u[3, 1] = 0x80000000
    u[4, 7] = 2
    return r   # (row 5 is valid)


def test_rows_outside_the_scene_are_left_alone(kat, host, oracle):
    r = refused_rows(kat)
    for got in (host.probe(io.STATE, r, fill=7.0)[0], io.oracle_probe(oracle, io.STATE, r[[0, 1, 2, 3, 5]], fill=7.0)[0]):
        assert (got[:-1] == 7.0).all() and (got[-1, :io.WORDS - 1] != 7.0).any()
    assert host.probe(io.SLOT, r)[1] == io.NO_DATA   # the host build keeps no shading lines


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------------
class Device:
    def __init__(self, scene):
        from vk_raytrace_amd import capi
        self.L = capi.lib()
        self.ctx = C.c_void_p()
        assert self.L.pt_create(0, C.byref(self.ctx)) == 0
        d, self.keep = scene.desc()
        assert self.L.pt_set_scene(self.ctx, C.byref(d)) == 0, self.L.pt_last_error(self.ctx)
        assert self.L.pt_build_accel(self.ctx) == 0, self.L.pt_last_error(self.ctx)

    def probe(self, kind, r, fill=np.nan):
        return io.call(self.L.pt_debug_surface_probe, (self.ctx,), kind, r, fill)

    def close(self):
        self.L.pt_destroy(self.ctx)


@pytest.fixture(scope="module")
def device(scene):
    d = Device(scene)
    yield d
    d.close()


@pytest.mark.gpu
def test_device_probe_is_the_host_builds(kat, device, host_out):
    for path in (0, 1):
        got, rc = device.probe(io.STATE, io.probe_rows(kat, path))
        assert rc == 0 and io.same_bits(got[:, :io.WORDS], host_out[path][:, :io.WORDS]) == 0, f"path {path}: device and host build differ"
    got, rc = device.probe(io.STATE, refused_rows(kat), fill=7.0)
    assert rc == 0 and (got[:-1] == 7.0).all() and (got[-1, :io.WORDS - 1] != 7.0).any()
    z, o = np.zeros((4, io.IN), np.float32), np.zeros((4, io.OUT), np.float32)
    fn = device.L.pt_debug_surface_probe
    assert fn(device.ctx, 2, 4, z.ctypes.data, io.IN, o.ctypes.data, io.OUT) < 0 and fn(device.ctx, 0, 4, z.ctypes.data, io.IN - 1, o.ctypes.data, io.OUT) < 0
    assert fn(device.ctx, 0, 4, z.ctypes.data, io.IN, o.ctypes.data, io.OUT - 1) < 0


@pytest.mark.gpu
def test_device_shading_lines_are_the_vertex_records(kat, scene, device):
    """SURF_SLOT over every slot of the flat structure: the (instance, primitive) pairs are a permutation of the scene's triangles, the six quads are the
    vertex records fetch_triangle reads for that pair (computed here from the packed vertex array), the material word is the instance's material index"""
    n = scene.num_triangles
    r = np.zeros((n + 2, io.IN), np.float32)
    r.view(np.uint32)[:, 0] = np.arange(n + 2)
    got, rc = device.probe(io.SLOT, r, fill=7.0)
    assert rc == 0 and (got[n:] == 7.0).all()   # slots past the last one are left alone
    ids = got[:n, 24:28].view(np.uint32)
    inst, prim = ids[:, 0].astype(np.int64), ids[:, 1].astype(np.int64)
    recs = kat["records"][kat["node_record"]]
    assert inst.max() < len(recs) and (prim < recs[inst][:, 3] // 3).all()
    assert len(set(zip(inst.tolist(), prim.tolist()))) == n == int((recs[:, 3] // 3).sum())
    assert np.array_equal(ids[:, 2].view(np.int32), recs[inst][:, 4]) and (ids[:, 3] == 0).all()
    verts = np.frombuffer(np.ascontiguousarray(scene.vertices).tobytes(), np.uint32).reshape(-1, 8)
    tri = kat["indices"][recs[inst][:, 2][:, None] + 3 * prim[:, None] + np.arange(3)[None, :]].astype(np.int64) + recs[inst][:, 0][:, None]
    assert np.array_equal(got[:n, :24].view(np.uint32), verts[tri].reshape(n, 24))


@pytest.mark.gpu
def test_debug_aov_frames_equal_the_oracle(scene, oracle):
    """one 32 x 24 frame per debug AOV on the fixture scene, the shipped kernels against the oracle bit for bit: ties the probe's path to shade_path's"""
    from tests.common import Config
    from vk_raytrace_amd.renderer import HipRenderer
    env = synth.procedural_sky(16, 8)
    cfg = Config(scene, env, 32, 24, depth=2)
    integral, _ = oracle.set_env(env)
    oracle.set_camera(cfg.camera)
    oracle.set_sunsky(cfg.sunsky)
    r = HipRenderer()
    r.setup(0)
    try:
        r.set_scene(scene)
        r.set_env(env)
        r.set_camera(cfg.camera)
        r.set_sunsky(cfg.sunsky)
        r.create((cfg.width, cfg.height))
        for name, mode in AOV_MODES.items():
            cfg.debug = mode
            st = cfg.state(integral)
            want = oracle.render(st, 1)
            st.frame = 0
            r.setPushContants(st)
            r.run(None, (cfg.width, cfg.height), None, None)
            got = r.read_accum()
            assert io.same_bits(got, want) == 0, f"{name}: {int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())} pixels differ from the oracle"
            if name == "alpha":
                assert (want[..., 0] > 0).mean() > 0.25   # the scene is in view
    finally:
        r.destroy()

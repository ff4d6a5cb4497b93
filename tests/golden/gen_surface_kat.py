"""Mints tests/golden/surface_kat.npz: a hit (instance, primitive, two barycentrics, a ray direction) turned into the shading state every BSDF call reads,
held to an INDEPENDENT model.

The HIP code (vk_raytrace_amd/csrc/pt_surface.h surface_at_hit / resolve_material / resolve_material_at), the CPU oracle (oracle/orc_path.h GetShadeState /
GetMaterialsAndTextures) and the compiled reference are compared bit for bit through whole frames only.  This file is the leg that shares nothing with them:
numpy only, written from the shader text
    shade_state.glsl:63-145            GetShadeState
    gltf_material.glsl:29-46           SRGBtoLINEAR (SRGB_FAST_APPROXIMATION: pow 2.2)
    gltf_material.glsl:52-93,104-193   GetMetallicRoughness, GetMaterialsAndTextures
    pathtrace.glsl:234-248             the State filled from the ShadeState, ffnormal, albedo *= colour
    compress.glsl:149-180              decompress_unit_vec: exact integers up to the final normalise (short_to_floatm11(v) = v / 32768 for |v| < 32768)
    common.glsl:80-92                  CreateCoordinateSystem
and evaluated twice, in float64 (the fixture's answer) and in float32 (decides, with the float64 one, which rows are KEPT).  Texture values come from the
numpy sampler model of gen_tex_kat.py (its address modes and its blend), not from any leg.  The inverse world matrix is computed in float64 from the
float32 matrix and rounded to float32, as pt_scene_records.cpp set_instance_transform and orc_scene.h build_world both do; it is an INPUT of both evaluations.

The scene is the smallest that reaches every line: five pieces of geometry of four triangles each (every vertex its own normal, tangent, handedness bit,
uv with the LSB of v set, colour; two triangles of a piece wound against their normals), the fourth holding the named edge cases, the fifth texture coordinates of
2^22, where the handedness bit is half a unit of v; seven instance classes (identity, translation to +-1e3, non-uniform scale from
{1/4, 1/2, 2, 4}, rotation about a skew axis, mirror, scale x rotation x mirror, a second rotated copy: every prim-mesh is instantiated seven times).  The
material is a property of the prim-mesh (host_device.h InstanceData.materialIndex), so the prim-mesh RECORDS are one per material and alias the five
pieces of geometry; one record has material -1 (-> material 0).

Rows.  One triangle per (record, instance) pair (stepping through the geometry's triangles), twelve points on it -- the three vertices, the three edge
midpoints, the centroid, five seeded interior points -- each with ONE ray direction: front side, back side or grazing (within 1e-3 of perpendicular to the
interpolated world normal), stepping with the point and the pair, so that every (point kind, ray kind) meets every material and every instance class.  (All
three directions on every point of every pair would be 12 k rows; their float64 results do not fit the size a committed fixture may have.)

Named edge rows (`row_edge` != 0) follow the shader as written; they are exempt from the tolerance leg and still compared bit for bit between the legs:
    1 tangent parallel to the normal   2 zero-area triangle   3 interpolated normal perpendicular to the geometric normal
    4 normal-map texel (0, 0, 0): the filtered value is exactly zero   5 anisotropy > 1 / 0.9 (sqrt of a negative number)   6 the all-ones normal code

Kept mask, decided by the model alone: a non-edge row is kept when its float32 and float64 evaluations agree within 1e-5 max(1, |value|) in every output
word and take every discrete decision alike (normal flip, ffnormal side before and after normal mapping, the branch of CreateCoordinateSystem, the eta
choice, the texel of every NEAREST tap).  Minting refuses when more than 2 % of the non-edge rows are dropped or a (record, instance) pair keeps fewer than 8 rows (the pairs
over the edge geometry and of the anisotropy > 1 / 0.9 material excepted: they hold the edge rows).

`simple`: per material, whether the product may shade it from its 128-byte line alone -- decided HERE from the rule in words (pt_device.h: "a material whose
remaining fields are the importer's defaults: no KHR transmission / clearcoat / sheen / anisotropy / volume, identity texture transform, lit"), bit for bit
against the default record, not by calling mat_is_simple.

BREAK: the rules of the model that tests/test_surface_model.py's docstring lists as broken one at a time to prove that the check can fail (main(path, brk)).

Run:  python tests/golden/gen_surface_kat.py   (rewrites surface_kat.npz; deterministic, byte-identical on every run)
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_tex_kat as tk  # noqa: E402  (the sampler model: wrap_modes, blend; words / uniform: deterministic inputs)

F32MAX = 3.402823466e+38
NEAREST, LINEAR = 0, 1
REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = 0, 1, 2
ROWS_PER_PAIR = 12
BREAK = ("h_vertex1", "lsb_kept", "no_flip", "ff_not_rederived", "scale_before_normalise", "mr_rg", "pow24", "clamp_dropped", "eta_inverted", "aspect_no09",
         "aniso_new_frame", "ccr_from_r", "uvt_colmajor", "scale_before_unpack")

# output words (vk_raytrace_amd/csrc/pt_probe.h surface_probe, SURF_STATE)
WORDS = 69
GROUPS = {  # name: (first word, count) -- the groups the tolerance is measured per
    "frame_position": (0, 3), "frame_normal": (3, 3), "frame_tangent": (6, 3), "frame_bitangent": (9, 3), "frame_uv": (12, 2), "frame_vcolor": (14, 3),
    "position": (17, 3), "normal": (20, 3), "ffnormal": (23, 3), "tangent": (26, 3), "bitangent": (29, 3), "uv": (32, 2), "albedo": (34, 3), "emission": (37, 3),
    "f0": (40, 3), "metallic": (43, 1), "roughness": (44, 1), "ax": (45, 1), "ay": (46, 1), "anisotropy": (47, 1), "clearcoat": (48, 1),
    "clearcoatRoughness": (49, 1), "transmission": (50, 1), "ior": (51, 1), "eta": (52, 1), "attenuationColor": (53, 3), "attenuationDistance": (56, 1),
    "alpha": (57, 1), "sheen": (58, 1), "sheenTint": (59, 3), "specular": (62, 1), "specularTint": (63, 1), "subsurface": (64, 1)}
INT_WORDS = (65, 66, 67)   # unlit, thinwalled, material index: exact.  (Word 68, the line path, is the product's own: `simple` names what it must be.)

MAT_DTYPE = np.dtype([  # host_device.h:133-179 GltfShadeMaterial, 216 bytes
    ("pbrBaseColorFactor", "<f4", 4), ("pbrBaseColorTexture", "<i4"), ("pbrMetallicFactor", "<f4"), ("pbrRoughnessFactor", "<f4"),
    ("pbrMetallicRoughnessTexture", "<i4"), ("emissiveTexture", "<i4"), ("_pad0", "<i4"), ("emissiveFactor", "<f4", 3), ("alphaMode", "<i4"),
    ("alphaCutoff", "<f4"), ("doubleSided", "<i4"), ("normalTexture", "<i4"), ("normalTextureScale", "<f4"), ("uvTransform", "<f4", 16), ("unlit", "<i4"),
    ("transmissionFactor", "<f4"), ("transmissionTexture", "<i4"), ("ior", "<f4"), ("anisotropyDirection", "<f4", 3), ("anisotropy", "<f4"),
    ("attenuationColor", "<f4", 3), ("thicknessFactor", "<f4"), ("thicknessTexture", "<i4"), ("attenuationDistance", "<f4"), ("clearcoatFactor", "<f4"),
    ("clearcoatRoughness", "<f4"), ("clearcoatTexture", "<i4"), ("clearcoatRoughnessTexture", "<i4"), ("sheen", "<u4"), ("_pad1", "<i4")])
assert MAT_DTYPE.itemsize == 216


def default_material():
    """the importer's defaults (src/scene.cpp:344-378 over nvh::GltfMaterial's)"""
    m = np.zeros((), MAT_DTYPE)
    m["pbrBaseColorFactor"] = 1.0
    m["pbrMetallicFactor"] = m["pbrRoughnessFactor"] = 1.0
    m["alphaCutoff"] = 0.5
    m["normalTextureScale"] = 1.0
    m["uvTransform"] = np.eye(4, dtype=np.float32).reshape(16)
    m["ior"] = 1.5
    m["anisotropyDirection"] = (0.0, 1.0, 0.0)
    m["attenuationColor"] = 1.0
    m["attenuationDistance"] = np.float32(F32MAX)
    for k in ("pbrBaseColorTexture", "pbrMetallicRoughnessTexture", "emissiveTexture", "normalTexture", "transmissionTexture", "thicknessTexture", "clearcoatTexture",
              "clearcoatRoughnessTexture"):
        m[k] = -1
    return m


def is_simple(m):
    """the rule in words of pt_device.h: every field but base colour factor / texture, metallic, roughness, their texture, emissive factor / texture, normal
    texture / scale, ior (and the alpha fields the shading does not read) is the importer's default, bit for bit; of uvTransform the two rows the shading reads"""
    d = default_material()
    same = lambda k: np.array_equal(np.atleast_1d(m[k]).view(np.uint32), np.atleast_1d(d[k]).view(np.uint32))
    uv = np.array_equal(m["uvTransform"][:8].view(np.uint32), d["uvTransform"][:8].view(np.uint32))
    return bool(uv and all(same(k) for k in ("unlit", "transmissionFactor", "transmissionTexture", "anisotropy", "anisotropyDirection", "attenuationColor",
                                              "thicknessFactor", "attenuationDistance", "clearcoatFactor", "clearcoatRoughness", "clearcoatTexture",
                                              "clearcoatRoughnessTexture", "sheen")))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a * b).sum(-1, keepdims=True)


def unit(a):
    return a / np.sqrt(dot(a, a))


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def decode_oct(code, dt):
    """compress.glsl:149-180: the integer part exactly, x y z / 32768 exactly, then the normalise in dt"""
    c = np.asarray(code, np.uint32).astype(np.int64)
    x, y = (c & 0xFFFF) - 32767, (c >> 16) - 32767
    mx, my = np.where(x < 0, -1, 0), np.where(y < 0, -1, 0)
    t0 = 32767 + mx + my
    ym = y ^ my
    t1 = t0 - (x ^ mx)
    z = t1 - ym
    neg = z < 0
    x, y = np.where(neg, (t0 - ym) ^ mx, x), np.where(neg, t1 ^ my, y)
    ones = c == 0xFFFFFFFF
    v = np.stack([x, y, z], 1)
    assert (np.abs(v[~ones]) < 32768).all()   # (short_to_floatm11 is linear only there)
    out = unit((v.astype(np.float64) / 32768.0).astype(dt))
    out[ones] = dt(F32MAX)
    return out


def sample(scene, tex, uv, dt, out_discrete):
    """textureLod(texturesMap[tex], uv, 0) per row (tex < 0: not sampled, zeros): Appendix F4 as gen_tex_kat models it -- x = u W (- 0.5), floor, fraction,
    the address mode on exact integers, the blend of the 0..255 values, / 255"""
    n = len(tex)
    out = np.zeros((n, 4), dt)
    zero = np.zeros(n, bool)   # the filtered RGB is exactly zero
    for t in np.unique(tex[tex >= 0]):
        m = tex == t
        img = scene[f"tex{t}"].astype(dt)
        h, w = img.shape[:2]
        mag, ws, wt = (int(v) for v in scene["tex_sampler"][t])
        lin = mag == LINEAR
        k = int(m.sum())
        foot = []
        for u, size, mode in ((uv[m, 0], w, ws), (uv[m, 1], h, wt)):
            x = u * dt(size)
            if lin:
                x = x - dt(0.5)
            i = np.floor(x)
            a = (x - i) if lin else np.zeros(k, dt)
            i = np.clip(i, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
            modes = np.full(k, mode)
            foot.append((tk.wrap_modes(i, size, modes), tk.wrap_modes(i + 1, size, modes) if lin else tk.wrap_modes(i, size, modes), a))
        (x0, x1, a), (y0, y1, b) = foot
        out[m] = tk.blend(img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1], a, b) / dt(255.0)
        zero[m] = (out[m][:, :3] == 0).all(1)
        if not lin:
            out_discrete.append((m, x0 + 65536 * y0))
    return out, zero


def model(scene, rows, dt, brk=None):
    """rows: dict of inst prim bu bv dir -> (out (n, WORDS) of dt with the integer words as VALUES, discrete decisions (n, k) int64, zero-texel mask)"""
    assert brk is None or brk in BREAK
    f = lambda a: np.asarray(a).astype(dt)
    inst, prim = rows["inst"].astype(np.int64), rows["prim"].astype(np.int64)
    n = len(inst)
    rec = scene["node_record"][inst].astype(np.int64)
    geo = scene["records"][rec]          # vertexOffset vertexCount firstIndex indexCount materialIndex
    tri = scene["indices"][(geo[:, 2][:, None] + 3 * prim[:, None] + np.arange(3)[None, :])].astype(np.int64) + geo[:, 0][:, None]
    mat = np.maximum(geo[:, 4], 0)       # shade_state.glsl:84
    M = scene["node_matrix"][inst].astype(np.float32)        # (n, 4, 4) row-major object -> world
    Minv = scene["node_inverse"][inst].astype(np.float32)    # (n, 3, 4) rows of the inverse
    M, Minv = f(M), f(Minv)
    bu, bv = f(rows["bu"])[:, None], f(rows["bv"])[:, None]
    b0 = (dt(1.0) - bu) - bv
    rdir = f(rows["dir"])
    disc = []

    P = f(scene["position"])[tri]        # (n, 3, 3)
    pos = P[:, 0] * b0 + P[:, 1] * bu + P[:, 2] * bv
    wpos = np.einsum("nij,nj->ni", M[:, :3, :3], pos) + M[:, :3, 3]
    with np.errstate(all="ignore"):
        N = [decode_oct(scene["normal_code"][tri[:, k]], dt) for k in range(3)]
        nrm = unit(N[0] * b0 + N[1] * bu + N[2] * bv)
        rowvec = lambda v: np.einsum("ni,nij->nj", v, Minv[:, :, :3])   # vec3(v * worldToObject): component j = dot(v, column j)
        wn = unit(rowvec(nrm))
        gn = unit(cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
        wg = unit(rowvec(gn))
        uvraw = scene["texcoord"][tri]       # (n, 3, 2) float32, LSB of v = handedness
        hv = 1 if brk == "h_vertex1" else 0
        h0 = np.where((uvraw[:, hv, 1].view(np.uint32) & 1) == 1, 1.0, -1.0).astype(dt)[:, None]
        T = [decode_oct(scene["tangent_code"][tri[:, k]], dt) for k in range(3)]
        tg = unit(T[0] * b0 + T[1] * bu + T[2] * bv)
        wt = unit(np.einsum("nij,nj->ni", M[:, :3, :3], tg))
        wt = unit(wt - dot(wt, wn) * wn)
        wb = cross(wn, wt) * h0
        vclr = uvraw.copy()
        if brk != "lsb_kept":
            vclr[:, :, 1] = (uvraw[:, :, 1].view(np.uint32) & np.uint32(0xFFFFFFFE)).view(np.float32)
        vclr = f(vclr)
        uv = vclr[:, 0] * b0 + vclr[:, 1] * bu + vclr[:, 2] * bv
        colb = scene["color_code"][tri]      # (n, 3) uint32 RGBA8
        col = [f(np.stack([(colb[:, k] >> s) & 0xFF for s in (0, 8, 16, 24)], 1)) / dt(255.0) for k in range(3)]
        color = (col[0] * b0 + col[1] * bu + col[2] * bv)[:, :3]
        flip = (dot(wn, wg) <= 0)[:, 0]
        if brk != "no_flip":
            wn = np.where(flip[:, None], -wn, wn)
        disc.append(flip)
        out = np.zeros((n, WORDS), dt)
        out[:, 0:3], out[:, 3:6], out[:, 6:9], out[:, 9:12], out[:, 12:14], out[:, 14:17] = wpos, wn, wt, wb, uv, color

        # pathtrace.glsl:234-245
        normal, tangent, bitangent = wn, wt, wb
        side0 = (dot(normal, rdir) <= 0)[:, 0]
        ffn = np.where(side0[:, None], normal, -normal)
        disc.append(side0)

        # gltf_material.glsl:104-193
        mt = scene["materials"][mat]
        mf = lambda k: f(mt[k])
        um = mf("uvTransform")
        if brk == "uvt_colmajor":
            uv = np.stack([uv[:, 0] * um[:, 0] + uv[:, 1] * um[:, 4] + um[:, 8] + um[:, 12], uv[:, 0] * um[:, 1] + uv[:, 1] * um[:, 5] + um[:, 9] + um[:, 13]], 1)
        else:   # vec4(uv, 1, 1) * M: component j = dot(v, column j), column j = words 4 j .. 4 j + 3
            uv = np.stack([uv[:, 0] * um[:, 0] + uv[:, 1] * um[:, 1] + um[:, 2] + um[:, 3], uv[:, 0] * um[:, 4] + uv[:, 1] * um[:, 5] + um[:, 6] + um[:, 7]], 1)
        T0, B0, N0 = tangent, bitangent, normal
        tbn = lambda v: T0 * v[:, 0:1] + B0 * v[:, 1:2] + N0 * v[:, 2:3]

        ntex = mt["normalTexture"].astype(np.int64)
        hasn = ntex > -1
        t, zero_texel = sample(scene, ntex, uv, dt, disc)
        s = mf("normalTextureScale")[:, None]
        scale3 = np.concatenate([s, s, np.ones_like(s)], 1)
        nv = (t[:, :3] * scale3 if brk == "scale_before_unpack" else t[:, :3]) * dt(2.0) - dt(1.0)
        nv = unit(nv * scale3) if brk == "scale_before_normalise" else (unit(nv) if brk == "scale_before_unpack" else unit(nv) * scale3)
        nn = unit(tbn(nv))
        normal = np.where(hasn[:, None], nn, normal)
        side1 = (dot(normal, rdir) <= 0)[:, 0]
        if brk != "ff_not_rederived":
            ffn = np.where(hasn[:, None], np.where(side1[:, None], normal, -normal), ffn)
        disc.append(np.where(hasn, side1, False))
        # CreateCoordinateSystem(ffnormal) (common.glsl:80-92)
        big = np.abs(ffn[:, 2]) > dt(0.99999)
        nt = unit(np.where(big[:, None], np.stack([-ffn[:, 0] * ffn[:, 1], dt(1.0) - ffn[:, 1] * ffn[:, 1], -ffn[:, 1] * ffn[:, 2]], 1),
                           np.stack([-ffn[:, 0] * ffn[:, 2], -ffn[:, 1] * ffn[:, 2], dt(1.0) - ffn[:, 2] * ffn[:, 2]], 1)))
        nb = cross(nt, ffn)
        tangent = np.where(hasn[:, None], nt, tangent)
        bitangent = np.where(hasn[:, None], nb, bitangent)
        disc.append(np.where(hasn, big, False))
        gamma = dt(2.4) if brk == "pow24" else dt(2.2)
        srgb = lambda c: np.concatenate([np.power(c[:, :3], gamma), c[:, 3:]], 1)

        emission = mf("emissiveFactor")
        etex = mt["emissiveTexture"].astype(np.int64)
        t, _ = sample(scene, etex, uv, dt, disc)
        emission = np.where((etex > -1)[:, None], emission * srgb(t)[:, :3], emission)

        ior = mf("ior")
        ds = (ior - dt(1.0)) / (ior + dt(1.0))
        ds = ds * ds
        rough, metal = mf("pbrRoughnessFactor"), mf("pbrMetallicFactor")
        mtex = mt["pbrMetallicRoughnessTexture"].astype(np.int64)
        t, _ = sample(scene, mtex, uv, dt, disc)
        cr, cm = (0, 1) if brk == "mr_rg" else (1, 2)
        rough = np.where(mtex > -1, t[:, cr] * rough, rough)
        metal = np.where(mtex > -1, t[:, cm] * metal, metal)
        base = mf("pbrBaseColorFactor")
        btex = mt["pbrBaseColorTexture"].astype(np.int64)
        t, _ = sample(scene, btex, uv, dt, disc)
        base = np.where((btex > -1)[:, None], base * srgb(t), base)
        f0 = ds[:, None] * (dt(1.0) - metal[:, None]) + base[:, :3] * metal[:, None]   # mix(x, y, a) = x (1 - a) + y a
        if brk != "clamp_dropped":
            rough = np.maximum(rough, dt(0.001))

        trans = mf("transmissionFactor")
        ttex = mt["transmissionTexture"].astype(np.int64)
        t, _ = sample(scene, ttex, uv, dt, disc)
        trans = np.where(ttex > -1, trans * t[:, 0], trans)

        inside = (dot(normal, ffn) > 0)[:, 0]
        if brk == "eta_inverted":
            inside = ~inside
        eta = np.where(inside, dt(1.0) / ior, ior)
        disc.append(inside)

        aniso = mf("anisotropy")
        aspect = np.sqrt(dt(1.0) - aniso * (dt(1.0) if brk == "aspect_no09" else dt(0.9)))
        gmax = lambda a, b: np.where(a < b, b, a)   # GLSL max(x, y) = x < y ? y : x
        ax, ay = gmax(np.full(n, dt(0.001)), rough / aspect), gmax(np.full(n, dt(0.001)), rough * aspect)
        adir = mf("anisotropyDirection")
        if brk == "aniso_new_frame":
            at = unit(tangent * adir[:, 0:1] + bitangent * adir[:, 1:2] + normal * adir[:, 2:3])
        else:
            at = unit(tbn(adir))
        ab = unit(cross(normal, at))
        tangent = np.where((aniso > 0)[:, None], at, tangent)
        bitangent = np.where((aniso > 0)[:, None], ab, bitangent)

        cc, ccr = mf("clearcoatFactor"), mf("clearcoatRoughness")
        ctex = mt["clearcoatTexture"].astype(np.int64)
        t, _ = sample(scene, ctex, uv, dt, disc)
        cc = np.where(ctex > -1, cc * t[:, 0], cc)
        rtex = mt["clearcoatRoughnessTexture"].astype(np.int64)
        t, _ = sample(scene, rtex, uv, dt, disc)
        ccr = np.where(rtex > -1, ccr * t[:, 0 if brk == "ccr_from_r" else 1], ccr)
        ccr = np.maximum(ccr, dt(0.001))
        sh = mt["sheen"].astype(np.uint32)
        sheen = f(np.stack([(sh >> s) & 0xFF for s in (0, 8, 16, 24)], 1)) / dt(255.0)

        o = out[:, 17:]
        o[:, 0:3], o[:, 3:6], o[:, 6:9], o[:, 9:12], o[:, 12:15], o[:, 15:17] = wpos, normal, ffn, tangent, bitangent, uv
        o[:, 17:20], o[:, 20:23], o[:, 23:26] = base[:, :3] * color, emission, f0
        o[:, 26], o[:, 27], o[:, 28], o[:, 29], o[:, 30], o[:, 31], o[:, 32], o[:, 33], o[:, 34], o[:, 35] = metal, rough, ax, ay, aniso, cc, ccr, trans, ior, eta
        o[:, 36:39], o[:, 39], o[:, 40], o[:, 41], o[:, 42:45] = mf("attenuationColor"), mf("attenuationDistance"), base[:, 3], sheen[:, 3], sheen[:, :3]
        o[:, 45], o[:, 46], o[:, 47] = dt(0.5), dt(1.0), dt(0.0)
        o[:, 48], o[:, 49], o[:, 50] = mt["unlit"] == 1, mt["thicknessFactor"] == 0, mat
    cols = []
    for d in disc:
        c = np.full(n, -1, np.int64)
        if isinstance(d, tuple):
            c[d[0]] = d[1]
        else:
            c = np.asarray(d).astype(np.int64)
        cols.append(c)
    return out, np.stack(cols, 1), zero_texel & hasn


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def encode_oct(v):
    """compress.glsl:111-139 (only used to CHOOSE codes: the model reads the codes, never the vectors they came from)"""
    v = np.asarray(v, np.float64)
    d = 32767.0 / np.abs(v).sum(1)
    x, y = np.rint(v[:, 0] * d).astype(np.int64), np.rint(v[:, 1] * d).astype(np.int64)
    neg = v[:, 2] < 0
    mx, my = np.where(x < 0, -1, 0), np.where(y < 0, -1, 0)
    tmp = 32767 + mx + my
    x2, y2 = (tmp - (y ^ my)) ^ mx, (tmp - (x ^ mx)) ^ my
    x, y = np.where(neg, x2, x), np.where(neg, y2, y)
    return (((y + 32767) << 16) | (x + 32767)).astype(np.uint32)


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def affine(m3, t=(0, 0, 0)):
    m = np.eye(4)
    m[:3, :3] = m3
    m[:3, 3] = t
    return m.astype(np.float32)


def inverse_rows(m):
    """the three rows of the inverse of the affine float32 matrix, in float64 (adjugate of the 3 x 3 part over its determinant), rounded to float32"""
    a = m.astype(np.float64)
    A, t = a[:3, :3], a[:3, 3]
    c = np.array([[A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1], A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2], A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]],
                  [A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2], A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0], A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]],
                  [A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0], A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1], A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]]])
    det = A[0, 0] * c[0, 0] + A[0, 1] * c[1, 0] + A[0, 2] * c[2, 0]
    inv = c / det
    return np.concatenate([inv, (-inv @ t)[:, None]], 1).astype(np.float32)


def instance_classes():
    R = rot((1.0, 2.0, 3.0), 0.7)
    S = np.diag([0.25, 2.0, 4.0])
    mirror = np.diag([-1.0, 1.0, 1.0])
    return [affine(np.eye(3)), affine(np.eye(3), (1000.0, -1000.0, 1000.0)), affine(S), affine(R), affine(mirror),
            affine(np.diag([0.5, 4.0, 2.0]) @ rot((3.0, -1.0, 2.0), 2.1) @ mirror, (3.0, -2.0, 5.0)), affine(rot((-2.0, 1.0, 0.5), 4.0), (-6.0, 1.0, 2.0))]


def perturbed(base, salt, amount):
    """unit vectors within about atan(amount sqrt 3) of the rows of base"""
    d = np.stack([tk.uniform(len(base), salt + k, -amount, amount) for k in range(3)], 1)
    v = base + d
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def geometry():
    """four pieces of four triangles, twelve vertices each (no vertex shared: every corner has its own attributes)"""
    pos, ncode, tcode, uv, col, idx, geo = [], [], [], [], [], [], []
    for g in range(5):
        p = np.stack([tk.uniform(12, 500 + 10 * g + k, -2.0, 2.0) for k in range(3)], 1).astype(np.float32).reshape(4, 3, 3)
        for t in range(4):   # triangles of a useful size: edges of about 1.5
            c = p[t].mean(0)
            p[t] = (c + (p[t] - c) * 0.8).astype(np.float32)
        if g == 3:
            p[0, 2] = p[0, 1]   # zero area: two corners in one place (the cross product of two equal edges is exactly zero)
        p = p.reshape(12, 3)
        tri = p.reshape(4, 3, 3).astype(np.float64)
        gn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        gn[np.linalg.norm(gn, axis=1) == 0] = (0.0, 0.0, 1.0)
        gn = np.repeat(gn / np.linalg.norm(gn, axis=1, keepdims=True), 3, 0)
        nrm = perturbed(gn, 600 + 10 * g, 0.35)       # within ~30 degrees of the geometric normal, different at every corner
        if g != 3:
            nrm[3:6], nrm[9:12] = -nrm[3:6], -nrm[9:12]  # triangles 1 and 3 are wound the other way round: their normals are moved to the geometric side
        e = np.repeat(tri[:, 1] - tri[:, 0], 3, 0)
        e[np.linalg.norm(e, axis=1) == 0] = (1.0, 0.0, 0.0)
        tan = e - nrm * (e * nrm).sum(1, keepdims=True)
        tan = perturbed(tan / np.linalg.norm(tan, axis=1, keepdims=True), 700 + 10 * g, 0.25)
        if g == 3:
            tan[6:9] = nrm[6:9]                                   # triangle 2: tangent parallel to the normal at every corner
            inplane = (tri[3, 1] - tri[3, 0]) / np.linalg.norm(tri[3, 1] - tri[3, 0])
            nrm[9:12] = inplane                                   # triangle 3: the normal lies in the triangle's plane
        nc, tc = encode_oct(nrm), encode_oct(tan)
        if g == 3:
            nc[4] = 0xFFFFFFFF                                    # triangle 1, vertex 1: the all-ones code
        u = np.stack([tk.uniform(12, 800 + 10 * g, -0.25, 1.75), tk.uniform(12, 801 + 10 * g, -0.25, 1.75)], 1).astype(np.float32)
        hand = (np.arange(12) % 3 + np.arange(12) // 3) % 2       # differs between the corners of a triangle; vertex 0 alternates over the triangles
        if g == 4:
            u[:, 1] = 2.0 ** 22   # far texture coordinates: the LSB of v is HALF A UNIT here, two rows of a four-row texture (anywhere near 1 it is an ulp, invisible)
        u[:, 1] = ((u[:, 1].view(np.uint32) & np.uint32(0xFFFFFFFE)) | hand.astype(np.uint32)).view(np.float32)
        c = tk.words(12, 900 + g)
        geo.append((len(np.concatenate(pos)) if pos else 0, 12, 12 * g, 12))
        pos.append(p); ncode.append(nc); tcode.append(tc); uv.append(u); col.append(c); idx.append(np.arange(12, dtype=np.uint32))
    # every triangle's vertex 0 .. 2 handedness bits differ; the LSB of v is set on at least one corner of every triangle
    return (np.concatenate(pos), np.concatenate(ncode), np.concatenate(tcode), np.concatenate(uv), np.concatenate(col).astype(np.uint32), np.concatenate(idx), geo)


def textures():
    """(image, (mag, wrapS, wrapT)).  0-2 normal maps (blue >= 160 keeps 2 t - 1 away from zero; one texel (0, 0, 0), one (255, 255, 255)), 3-6 colour data with
    a 0 and a 255 in every channel.  1 and 6 have the same size and sampler (an interleaved group where one material uses both)."""
    out = []
    specs = [(4, 4, NEAREST, REPEAT, REPEAT, True), (8, 4, LINEAR, REPEAT, REPEAT, True), (5, 3, NEAREST, MIRRORED_REPEAT, CLAMP_TO_EDGE, True),
             (4, 4, LINEAR, MIRRORED_REPEAT, REPEAT, False), (8, 4, NEAREST, REPEAT, REPEAT, False), (5, 3, LINEAR, CLAMP_TO_EDGE, MIRRORED_REPEAT, False),
             (8, 4, LINEAR, REPEAT, REPEAT, False)]
    for t, (w, h, mag, ws, wt, nmap) in enumerate(specs):
        img = tk.words(w * h, 1100 + t).view(np.uint8).reshape(h, w, 4).copy()
        if nmap:
            img[:, :, 2] = 160 + img[:, :, 2] % 96
            img[h - 1, w - 1] = (0, 0, 0, 255)
        else:
            img[h - 1, w - 1] = (0, 0, 0, 0)
        img[0, 0] = (255, 255, 255, 255)
        out.append((img, (mag, ws, wt)))
    return out


def materials():
    """(name, record); the order is the material index"""
    out = []

    def add(name, **kw):
        m = default_material()
        m["pbrBaseColorFactor"] = (0.8, 0.6, 0.4, 0.9)
        m["pbrMetallicFactor"], m["pbrRoughnessFactor"] = 0.7, 0.45
        m["emissiveFactor"] = (0.5, 0.25, 1.5)
        for k, v in kw.items():
            if k.startswith("uvT"):
                m["uvTransform"][int(k[3:])] = v
            else:
                m[k] = v
        out.append((name, m))

    N, E, MR, B = dict(normalTexture=0), dict(emissiveTexture=3), dict(pbrMetallicRoughnessTexture=5), dict(pbrBaseColorTexture=4)
    add("plain")
    add("normal", **N); add("emissive", **E); add("metallic-roughness", **MR); add("base colour", **B)
    add("all four", normalTexture=1, emissiveTexture=6, pbrMetallicRoughnessTexture=3, pbrBaseColorTexture=5)
    for k in range(8):
        add(f"uvTransform[{k}]", pbrBaseColorTexture=3, **{f"uvT{k}": (1.25, 0.25, 0.125, -0.375, -0.25, 0.75, 0.5, 0.0625)[k]})
    add("transmission -0.0", transmissionFactor=np.float32(-0.0))
    add("transmission texture", transmissionTexture=6)
    add("anisotropy", anisotropy=0.25)
    add("anisotropy direction", anisotropyDirection=(0.6, 0.8, 0.0))
    for k in range(3):
        c = [1.0, 1.0, 1.0]
        c[k] = 0.5
        add(f"attenuation colour {k}", attenuationColor=tuple(c))
    add("thickness", thicknessFactor=0.5)
    add("attenuation distance", attenuationDistance=2.0)
    add("clearcoat", clearcoatFactor=0.5)
    add("clearcoat roughness", clearcoatRoughness=0.3)
    add("clearcoat texture", clearcoatTexture=3)
    add("clearcoat roughness texture", clearcoatRoughnessTexture=5)
    add("sheen", sheen=0xFF000000)
    add("unlit", unlit=1)
    # values
    add("normal scale 0.5", normalTexture=1, normalTextureScale=0.5)
    add("normal scale 2", normalTexture=2, normalTextureScale=2.0)
    add("roughness 0", pbrRoughnessFactor=0.0)
    add("clearcoat roughness 0", clearcoatFactor=1.0, clearcoatRoughness=0.0)
    add("ior 1", ior=1.0)
    add("ior 2.4", ior=2.4)
    add("anisotropy 0.5 + normal map", anisotropy=0.5, anisotropyDirection=(0.6, 0.8, 0.0), normalTexture=0)
    add("anisotropy 1", anisotropy=1.0, anisotropyDirection=(0.8, -0.6, 0.0))
    add("sheen four bytes", sheen=0x80C04020)
    add("transmission 0.75 x texture", transmissionFactor=0.75, transmissionTexture=4)
    add("clearcoat x textures", clearcoatFactor=0.8, clearcoatRoughness=0.6, clearcoatTexture=6, clearcoatRoughnessTexture=6)
    add("roughness texture to the clamp", pbrRoughnessFactor=0.003, pbrMetallicRoughnessTexture=3)
    add("everything", normalTexture=1, emissiveTexture=6, pbrMetallicRoughnessTexture=4, pbrBaseColorTexture=3, transmissionFactor=0.5, transmissionTexture=5,
        anisotropy=0.6, anisotropyDirection=(0.28, 0.96, 0.0), clearcoatFactor=0.9, clearcoatRoughness=0.4, clearcoatTexture=3, clearcoatRoughnessTexture=4,
        sheen=0x10204080, attenuationColor=(0.9, 0.5, 0.2), attenuationDistance=0.5, thicknessFactor=0.1, ior=1.33, normalTextureScale=1.5,
        uvT0=0.75, uvT1=0.25, uvT3=0.125, uvT4=-0.25, uvT5=1.5, uvT6=0.0625)
    add("anisotropy 1.25", anisotropy=1.25)   # > 1 / 0.9: edge
    return out


def build_scene():
    pos, ncode, tcode, uv, col, idx, geo = geometry()
    scene = dict(position=pos, normal_code=ncode, tangent_code=tcode, texcoord=uv, color_code=col, indices=idx)
    with np.errstate(all="ignore"):
        scene["normal"] = decode_oct(ncode, np.float64).astype(np.float32)           # the raw attributes the codes stand for
        scene["tangent"] = np.concatenate([decode_oct(tcode, np.float64), np.where((uv[:, 1].view(np.uint32) & 1) == 1, 1.0, -1.0)[:, None]], 1).astype(np.float32)
    scene["color"] = (np.stack([(col >> s) & 0xFF for s in (0, 8, 16, 24)], 1) / 255.0).astype(np.float32)
    tex = textures()
    for t, (img, _) in enumerate(tex):
        scene[f"tex{t}"] = img
    scene["tex_sampler"] = np.array([s for _, s in tex], np.int32)
    mats = materials()
    scene["materials"] = np.array([m for _, m in mats], MAT_DTYPE)
    scene["material_names"] = np.array([nm for nm, _ in mats])
    scene["simple"] = np.array([is_simple(m) for _, m in mats])
    recs, rec_geo = [], []
    for m in range(len(mats)):   # one prim-mesh record per material over the three plain pieces of geometry
        g = m % 3
        recs.append(geo[g] + (m,)); rec_geo.append(g)
    recs.append(geo[0] + (-1,)); rec_geo.append(0)                  # no material: index -1 -> material 0
    for m in (0, 5):                                                # the edge geometry, plain and with all four textures
        recs.append(geo[3] + (m,)); rec_geo.append(3)
    recs.append(geo[4] + (4,)); rec_geo.append(4)                   # the far texture coordinates under the NEAREST base-colour texture
    scene["records"] = np.array(recs, np.int32)
    scene["record_geometry"] = np.array(rec_geo, np.int32)
    classes = instance_classes()
    node_rec, node_cls, mats4 = [], [], []
    for r in range(len(recs)):
        for c, m in enumerate(classes):
            node_rec.append(r); node_cls.append(c)
            mm = m.copy()
            mm[:3, 3] += np.float32(3.0) * np.array([r % 8 - 3.5, (r // 8) % 8 - 3.5, 0.0], np.float32)   # (the records side by side: a frame sees many of them)
            mats4.append(mm)
    scene["node_record"], scene["node_class"] = np.array(node_rec, np.int32), np.array(node_cls, np.int32)
    scene["node_matrix"] = np.array(mats4, np.float32)
    scene["node_inverse"] = np.array([inverse_rows(m) for m in mats4], np.float32)
    return scene


def build_rows(scene):
    nn = len(scene["node_record"])
    inst = np.repeat(np.arange(nn), ROWS_PER_PAIR)
    j = np.tile(np.arange(ROWS_PER_PAIR), nn)
    prim = (inst + inst // 7) % 4
    edge_geo = scene["record_geometry"][scene["node_record"][inst]] == 3
    prim = np.where(edge_geo, (inst % 7 + j) % 4, prim)   # the edge geometry: every one of its triangles on every instance
    n = len(inst)
    canon = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0.5, 0.5], [0, 0.5], [1 / 3, 1 / 3]])
    a, b = tk.uniform(n, 41, 0.02, 0.98), tk.uniform(n, 42, 0.02, 0.98)
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    far = scene["record_geometry"][scene["node_record"][inst]] == 4
    pt = np.where(far, j % 6, j)   # far texture coordinates: vertices and edge midpoints only (weights 0, 1/2, 1: float32 interpolates a coordinate of 2^22 exactly there)
    bu = np.where(pt < 7, canon[np.minimum(pt, 6), 0], a).astype(np.float32)
    bv = np.where(pt < 7, canon[np.minimum(pt, 6), 1], b).astype(np.float32)
    rows = dict(inst=inst.astype(np.int32), prim=prim.astype(np.int32), bu=bu, bv=bv, dir=np.zeros((n, 3), np.float32))
    # the ray: against the interpolated world normal of the float64 model (front), along it (back), or across it, 1e-3 off perpendicular (grazing)
    with np.errstate(all="ignore"):
        o, _, _ = model(scene, rows, np.float64)
    wn, wt = o[:, 3:6], o[:, 6:9]
    bad = ~np.isfinite(wn).all(1) | ~np.isfinite(wt).all(1)
    wn, wt = np.where(bad[:, None], (0.0, 0.0, 1.0), wn), np.where(bad[:, None], (1.0, 0.0, 0.0), wt)
    side = np.stack([tk.uniform(n, 43 + k, -0.5, 0.5) for k in range(3)], 1)
    kind = (j + inst) % 3
    sgn = np.where((j // 3 + inst) % 2 == 0, 1.0, -1.0)[:, None]
    d = np.where((kind == 0)[:, None], -wn + side, np.where((kind == 1)[:, None], wn + side, wt + 0.3 * np.cross(wn, wt) + sgn * 1e-3 * wn))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rows["dir"] = d.astype(np.float32)
    rows["kind"] = kind.astype(np.int8)
    return rows


def edge_kinds(scene, rows, zero_texel):
    rec = scene["node_record"][rows["inst"]]
    edge = np.zeros(len(rec), np.int8)
    g3 = scene["record_geometry"][rec] == 3
    edge[zero_texel] = 4
    mat = np.maximum(scene["records"][rec][:, 4], 0)
    edge[scene["materials"]["anisotropy"][mat] > 1 / 0.9] = 5
    for prim, kind in ((0, 2), (1, 6), (2, 1), (3, 3)):
        edge[g3 & (rows["prim"] == prim)] = kind
    return edge


def evaluate(scene, rows, brk=None):
    with np.errstate(all="ignore"):
        o64, d64, zero = model(scene, rows, np.float64, brk)
        o32, d32, _ = model(scene, rows, np.float32, brk)
    edge = edge_kinds(scene, rows, zero)
    fw = [w for w in range(WORDS - 1) if w not in INT_WORDS]
    with np.errstate(all="ignore"):
        close = np.abs(o32[:, fw].astype(np.float64) - o64[:, fw]) <= 1e-5 * np.maximum(1.0, np.abs(o64[:, fw]))
    kept = close.all(1) & (d32 == d64).all(1) & (o32[:, list(INT_WORDS)] == o64[:, list(INT_WORDS)]).all(1) & (edge == 0)
    return o64, kept, edge


def write_npz(path, out):
    with zipfile.ZipFile(path, "w") as z:   # like np.savez_compressed, with a fixed timestamp: the same bytes on every run
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main(path=None, brk=None):
    scene = build_scene()
    rows = build_rows(scene)
    want, kept, edge = evaluate(scene, rows, brk)
    plain = edge == 0
    dropped = 1.0 - kept[plain].mean()
    assert dropped <= 0.02, f"{dropped:.2%} of the non-edge rows dropped"
    pair_kept = np.bincount(rows["inst"][kept], minlength=len(scene["node_record"]))
    pair_edge = np.bincount(rows["inst"][~plain], minlength=len(scene["node_record"]))
    node_mat = np.maximum(scene["records"][scene["node_record"]][:, 4], 0)
    need = (scene["record_geometry"][scene["node_record"]] != 3) & ~(scene["materials"]["anisotropy"][node_mat] > 1 / 0.9)   # (those pairs hold edge rows instead)
    assert (pair_kept[need] >= 8).all(), ("a (record, instance) pair keeps fewer than 8 rows", np.nonzero(need & (pair_kept < 8))[0][:8])
    assert all((edge == k).sum() >= 4 for k in range(1, 7)), np.bincount(edge)
    out = dict(scene)
    for k, v in rows.items():
        out["row_" + k] = v
    out["row_edge"], out["row_kept"] = edge, kept
    out["want"] = np.ascontiguousarray(want.T)   # (WORDS, rows): a word's column is contiguous (equal columns and constant runs then compress)
    out["group_names"] = np.array(list(GROUPS))
    out["group_words"] = np.array(list(GROUPS.values()), np.int32)
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "surface_kat.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(kept), "rows,", int(kept.sum()), "kept,", int((~plain).sum()), "edge,", f"{dropped:.3%} dropped,",
          len(scene["materials"]), "materials,", len(scene["node_record"]), "instances")


if __name__ == "__main__":
    main(*sys.argv[1:3])

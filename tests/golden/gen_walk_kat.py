"""Mints tests/golden/walk_kat.npz: the candidate walk of the trace contract and stochastic alpha held to an INDEPENDENT model.

The layers under the walk have models of their own (gen_trace_kat.py: T1 / T2 and the box tests; gen_tex_kat.py: the sampler; gen_kat.py: tea and pcg).  This file
is the walk itself, per ray a brute force over every world triangle, written from the shader text and the host rules it restates
    traceray_rq.glsl:32-102    HitTest: the base-colour alpha, the uv transform, MASK `>` cutoff, ONE draw, rejected iff rand > opacity
    traceray_rq.glsl:108-147   ClosestHit: unbounded, back faces culled, the candidates a driver reports are confirmed or not by HitTest
    traceray_rq.glsl:153-185   AnyHit: the same loop bounded by maxDist; the ray-query flavour draws from prd.seed itself
    traceray_rtx.glsl:54-55    the RTX flavour's shadow ray draws from a copy: the caller's seed comes back untouched
    accelstruct.cpp:144-149    an instance is opaque when alphaMode == 0, or baseColorFactor.a == 1 with no base-colour texture; culling is off for doubleSided == 1
    DESIGN.md 3                T4, which the reference leaves to the driver: candidates in the order of the key (t, world index)
It imports numpy, the standard library and the other generators of this directory only; nothing of oracle/, tests/orc.py, tests/host_harness.py or vk_raytrace_amd/.

The model.  World triangles by T1's bit contract (gen_trace_kat.xform_bits on the node matrix, edges taken in world space: nine fp32 words per triangle).  T2 in
float64 on those words, in the contract's expression tree.  T3 from the sign of det, flipped where the float64 determinant of the node matrix is negative, skipped
for doubleSided == 1.  T4: accepted candidates (u >= 0, v >= 0, u + v <= 1, t > 0) sorted by (t, world index).  Opacity: gen_tex_kat.axis / blend on the
interpolated, uv-transformed coordinate, times the fp32 factor, `>` cutoff for MASK.  Draws: gen_kat's pcg, one per non-opaque candidate in key order, rejected iff
rand > opacity.  T5: opaque commits without a draw, the walk ends at the first commit.  T6: the same walk over the keys in (0, tmax), upper bound exclusive; the
verdict is "any commit"; the seed comes back advanced (ray query) or untouched (RTX).  Any-hit off: every triangle is opaque, nothing draws.

Kept mask, decided by the model alone.  A ray is kept when the float32 and the float64 evaluation of the model take every decision alike and
  * no triangle that faces the ray has it within EDGE (barycentric) of one of its edges, and |det| > 2 B(det) on every triangle it meets;
  * consecutive keys are SEP max(1, t) apart, or TIED: the two triangles' nine record words are bit-identical (then t is, and the world index decides);
  * no key lies within SEP max(1, tmax) of a bounded ray's end or within TZERO of its origin (EDGE, SEP, TZERO are gen_path_kat's);
  * every MASK threshold and every rand-against-opacity comparison is decided by an interval: with B the running-error bound of gen_trace_kat's V arithmetic
    (restated here for numpy arrays), the texture coordinate is known to E = |uv0| B(1-u-v) + |uv1| B(u) + |uv2| B(v) plus eight roundings, through the transform;
    a LINEAR tap moves by at most one unit per texel and axis (bilinear filtering is continuous and blends values at most 1 apart), so the opacity lies within
    |factor| (E_x W + E_y H + (|x W| + |y H| + 4) 2^-23) of the model's, gen_tex_kat's LINEAR bound included; a NEAREST tap must name its texel (the coordinate is
    farther from a texel edge than E W + |x W| 2^-23), then 4 2^-23 |factor|.  The cutoff, or the draw, must lie outside that interval.  An untextured
    material's opacity is its fp32 factor: the interval is a point, and a draw is a dyadic rational, so the comparison is exact.
The exact rows and the zero-draw rays are kept by construction: every operation of T2 on every candidate they meet is exact in fp32 (asserted here through
gen_trace_kat.t2_truth, fractions.Fraction), their candidates are untextured or compared with a draw of 0.0 against an opacity of about 1, and their margins to
`tmax` are the point of the row.

The 0.0 draw.  rand returns exactly 0.0 iff word >> 9 == 0, one state in 2^23.  zero_states() scans successor states upward from 0 until it has 8 of them and inverts
the affine step (747796405 is odd) once or twice: seeds whose first, or second, draw is 0.0.  `!(0.0 > 0.0)`: a zero-opacity candidate that draws 0.0 COMMITS.

Caps, asserted here and again by the test: at most 10 % of the rays of any family dropped; at least 50 kept rays per tag of TAGS, 4 for the exact-row and zero-draw
tags.  Census of the committed fixture (kept rays per tag), as printed by this file:
    rays 4396 triangles 200
    dropped per family: eye cloud 1.5%, surface to surface 0.7%, coincident pairs 0.0%, staircases 0.0%, exact rows 0.0%, zero draws 0.0%
    kept rays per tag:
    zero in front: 0 2466; zero in front: 1 926; zero in front: 2 601; zero in front: 3 168; zero in front: more than 3 205; zero behind: 0 1914;
    zero behind: 1 848; zero behind: 2 479; zero behind: 3 177; zero behind: more than 3 110; zero on both sides of the hit 662;
    fractional candidate walked 619; MASK texel in a uniform block 269; MASK texel in a mixed block 288; general tap 76; uvTransform with rotation 104;
    tie (zero, opaque) 98; tie (opaque, zero) 94; tie (fractional, fractional) 183; tie (zero, zero) 241; mirrored instance culled 116;
    mirrored instance accepted 65; opaque by rule 134; shadow ray ended by tmax 1554; shadow draws (RTX differs) 1812; BLAS instance committed 128;
    merged structure committed 3400; miss 838; 0.0 on a zero-opacity candidate, closest 116; 0.0 on a zero-opacity candidate, shadow 116;
    0.0 on the certain hit's own draw 60; exact row: tmax = t 40; exact row: tmax = nextafter(t) 40; exact row: tmax <= 0 40

BREAK: the rules tools/walk_mutations.py breaks in the product one at a time, broken here in the model instead (main(path, brk)); tests/test_walk_model.py checks
that each makes the model disagree with the committed fixture.

Run:  python tests/golden/gen_walk_kat.py   (rewrites walk_kat.npz; deterministic, byte-identical on every run)
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_surface_kat as gs  # noqa: E402
import gen_tex_kat as tk  # noqa: E402
import gen_trace_kat as gt  # noqa: E402
from gen_path_kat import EDGE, SEP, TZERO  # noqa: E402

OUT = os.path.join(HERE, "walk_kat.npz")
INF = np.float32(1e32)   # globals.glsl:29; what the C ABI takes for "unbounded"
U, ETA = 2.0 ** -24, 2.0 ** -149
KEYS = 16                # CANDIDATES results per ray
OPAQUE, MASK, BLEND = 0, 1, 2   # host_device.h ALPHA_*
FAMILIES = ("eye cloud", "surface to surface", "coincident pairs", "staircases", "exact rows", "zero draws")
F_EYE, F_SURF, F_PAIR, F_STAIR, F_EXACT, F_ZERO = range(6)
BREAK = ("tie_desc", "reject_ge", "mask_ge", "flip_ignored", "tmax_inclusive", "rtx_seed_written", "opaque_rule_no_arm", "opaque_draws", "zero_never_commits",
         "count_excludes_ties")
TAGS = ("zero in front: 0", "zero in front: 1", "zero in front: 2", "zero in front: 3", "zero in front: more than 3",
        "zero behind: 0", "zero behind: 1", "zero behind: 2", "zero behind: 3", "zero behind: more than 3", "zero on both sides of the hit",
        "fractional candidate walked", "MASK texel in a uniform block", "MASK texel in a mixed block", "general tap", "uvTransform with rotation",
        "tie (zero, opaque)", "tie (opaque, zero)", "tie (fractional, fractional)", "tie (zero, zero)",
        "mirrored instance culled", "mirrored instance accepted", "opaque by rule", "shadow ray ended by tmax", "shadow draws (RTX differs)",
        "BLAS instance committed", "merged structure committed", "miss",
        "0.0 on a zero-opacity candidate, closest", "0.0 on a zero-opacity candidate, shadow", "0.0 on the certain hit's own draw",
        "exact row: tmax = t", "exact row: tmax = nextafter(t)", "exact row: tmax <= 0")
SMALL_TAGS = TAGS[-6:]   # at least 4 kept rays; every other tag at least 50
TAG = {name: np.uint64(1) << np.uint64(k) for k, name in enumerate(TAGS)}


# ---- the fixture scene -----------------------------------------------------------------------------------------------------------------------------------
MATERIALS = ("wall", "zero", "frac", "frac2", "texfrac", "one", "above", "maskpot", "masknpot", "maskhi", "masklo", "maskrule", "opaquetex", "zero_ss", "opaque_ss",
             "texrot", "maskpot_ss", "frac_ss", "maskeq")
M = {name: k for k, name in enumerate(MATERIALS)}


def textures():
    """(image (h, w, 4) bytes, (mag, wrapS, wrapT)); only alpha matters to the walk"""
    def img(w, h, salt):
        return tk.words(w * h, salt).view(np.uint8).reshape(h, w, 4).copy()
    t0 = img(8, 8, 3100)
    t0[:, :, 3] = 40 + t0[:, :, 3] % 176            # 40 .. 215: under a factor of 0.875 always fractional
    t1 = img(4, 4, 3101)
    t1[:, :, 3] = 255
    t2 = img(16, 16, 3102)                          # 4 x 4-texel blocks, REPEAT on a power of two: opacity-map blocks ZERO, ONE and UNKNOWN
    t2[0:8, 0:8, 3] = 0
    t2[0:8, 8:16, 3] = 255
    t2[8:16, 0:8, 3] = np.where((np.add.outer(np.arange(8), np.arange(8)) % 2) == 0, 127, 128)   # either side of the cutoff 0.5: 127 / 255 < 0.5 < 128 / 255
    t3 = img(5, 3, 3103)                            # not a power of two, CLAMP: the general tap
    t4 = img(4, 4, 3104)
    t4[:, :, 3] = 0
    return [(t0, (tk.LINEAR, tk.REPEAT, tk.REPEAT)), (t1, (tk.NEAREST, tk.REPEAT, tk.REPEAT)), (t2, (tk.LINEAR, tk.REPEAT, tk.REPEAT)),
            (t3, (tk.LINEAR, tk.CLAMP_TO_EDGE, tk.CLAMP_TO_EDGE)), (t4, (tk.NEAREST, tk.REPEAT, tk.REPEAT))]


def materials():
    out = []

    def add(name, mode, a, tex=-1, ds=1, cutoff=0.5, rot=None):
        assert M[name] == len(out)
        m = gs.default_material()
        m["pbrMetallicFactor"] = 0.0
        m["pbrBaseColorFactor"] = (0.8, 0.7, 0.6, a)
        m["alphaMode"], m["alphaCutoff"], m["pbrBaseColorTexture"], m["doubleSided"] = mode, cutoff, tex, ds
        if rot is not None:   # vec4(uv, 1, 1) * M: x = u m0 + v m1 + m2 + m3, y = u m4 + v m5 + m6 + m7
            c, s = np.cos(rot), np.sin(rot)
            m["uvTransform"][:8] = (c, s, 0.25, 0.0, -s, c, 0.5, 0.0)
        out.append(m)

    add("wall", OPAQUE, 1.0)
    add("zero", BLEND, 0.0)
    add("frac", BLEND, 0.375)
    add("frac2", BLEND, 0.625)
    add("texfrac", BLEND, 0.875, tex=0)
    add("one", BLEND, 1.0, tex=1)                  # the product is exactly 1
    add("above", BLEND, 1.5, tex=1)
    add("maskpot", MASK, 1.0, tex=2)
    add("masknpot", MASK, 0.9, tex=3, cutoff=0.4)
    add("maskhi", MASK, 0.75)                      # untextured, factor != 1: opacity 1, and a draw
    add("masklo", MASK, 0.25)                      # opacity 0
    add("maskrule", MASK, 1.0)                     # factor 1 and no texture: opaque by the rule, draws nothing
    add("opaquetex", OPAQUE, 0.5, tex=4)           # alphaMode OPAQUE over a texture of alpha 0: opaque, never evaluated
    add("zero_ss", BLEND, 0.0, ds=0)
    add("opaque_ss", OPAQUE, 1.0, ds=0)
    add("texrot", BLEND, 0.875, tex=0, rot=0.6)
    add("maskpot_ss", MASK, 1.0, tex=2, ds=0)
    add("frac_ss", BLEND, 0.375, ds=0)
    add("maskeq", MASK, 0.5)                       # factor == cutoff: `>` says 0
    return np.array(out, gs.MAT_DTYPE)


COLS_X, ROW_IN, ROW_OUT = (-6.0, -3.0, 0.0, 3.0, 6.0), (-2.0, 2.0), 6.0
FULL = (-1.0, 1.0)        # a card is 2 x 2 or a power-of-two part of it, a wall cell 4 x 2: 1 / det is an fp32 number on an axis-parallel ray (the exact rows)
STEPS = (-1.0, 0.0, 0.5, 0.75, 0.875)


def stairs(sign, mat, axis, facing=1):
    """five cards at |z| = 1 .. 5; the card at |z| = k starts at STEPS[k - 1] along `axis`: a ray meets 1 .. 5 of them"""
    return [(sign * k, mat, (STEPS[k - 1], 1.0) if axis == 0 else FULL, FULL if axis == 0 else (STEPS[k - 1], 1.0), facing) for k in range(1, 6)]


def columns():
    """(cx, cy, [(z, material or (material, material) for a coincident pair, x range, y range, facing +-1)])"""
    c = []
    X, (Y0, Y1), YO = COLS_X, ROW_IN, ROW_OUT
    c.append((X[0], Y0, stairs(1, "zero", 0) + stairs(-1, "zero", 1)))
    c.append((X[1], Y0, [(5, "zero", FULL, FULL, 1), (4, "frac", (-0.5, 1.0), FULL, 1), (3, "texfrac", (0.0, 1.0), FULL, 1), (2, "one", (0.5, 1.0), FULL, 1),
                         (1, "above", (-1.0, 0.5), FULL, 1), (-6, "masklo", FULL, FULL, 1), (-5, "maskpot", FULL, FULL, 1), (-4, "masknpot", (-0.5, 1.0), FULL, 1),
                         (-3, "maskhi", (0.0, 0.5), FULL, 1), (-2, "maskrule", (0.5, 1.0), FULL, 1), (-1, "opaquetex", (-1.0, -0.5), FULL, 1)]))
    c.append((X[2], Y0, [(3, "zero", FULL, FULL, 1), (2, "zero", (0.0, 1.0), FULL, 1), (1, "frac", FULL, FULL, 1),
                         (-1, "texrot", FULL, FULL, 1), (-2, "maskeq", FULL, (0.0, 1.0), 1), (-3, "maskpot", FULL, FULL, 1)]))
    c.append((X[3], Y0, [(2, "zero", (0.0, 1.0), FULL, 1), (1, "one", FULL, FULL, 1), (-1, "maskhi", FULL, FULL, 1), (-2, "zero", (0.0, 1.0), FULL, 1),
                         (-3, "above", (-1.0, 0.0), FULL, 1)]))
    c.append((X[4], Y0, [(2, ("zero", "wall"), FULL, FULL, 1), (-2, ("wall", "zero"), FULL, FULL, 1)]))
    c.append((X[0], Y1, [(2, ("frac", "frac2"), FULL, FULL, 1), (-2, ("frac2", "frac"), FULL, FULL, 1)]))
    c.append((X[1], Y1, [(2, ("zero", "masklo"), FULL, FULL, 1), (-2, ("masklo", "zero"), FULL, FULL, 1)]))
    c.append((X[3], Y1, [(2, "texfrac", FULL, FULL, 1), (1, "maskpot", FULL, FULL, 1), (-1, "masknpot", FULL, FULL, 1), (-2, "texrot", FULL, FULL, 1),
                         (-3, "maskrule", (0.0, 1.0), FULL, 1), (-3, "opaquetex", (-1.0, 0.0), FULL, 1)]))
    c.append((X[4], Y1, stairs(1, "zero_ss", 1) + stairs(-1, "zero_ss", 0, facing=-1)))
    # beyond the wall's edge: seen from both sides, and a ray that passes everything misses
    c.append((X[0], YO, [(2, "zero_ss", FULL, FULL, 1), (-2, "opaque_ss", FULL, FULL, 1)]))
    c.append((X[3], YO, [(1, "frac", FULL, FULL, 1), (0, "maskpot", FULL, FULL, 1), (-1, "zero", FULL, FULL, 1), (-2, "frac_ss", FULL, FULL, -1)]))
    c.append((X[4], YO, stairs(1, "zero", 0) + [(0, "opaque_ss", FULL, FULL, -1)]))
    return c


INSTANCED_AT = (COLS_X[2], ROW_IN[1], 2.0)          # the thrice-instantiated mesh itself (its first node's matrix is the identity)
ROTATED_AT, MIRRORED_AT = (COLS_X[2], ROW_OUT, 0.5), (COLS_X[1], ROW_OUT, 1.0)
EXACT_DX, EXACT_DY = (-0.625, -0.375, 0.125, 0.625, 0.9375), (0.375, -0.5625, 0.3125, -0.125, 0.8125)   # dyadic, off every card edge and diagonal


def build_scene():
    pos, uv, idx, recs, nodes, kinds = [], [], [], [], [], []
    eye4 = np.eye(4, dtype=np.float32)

    def grid(p0, e1, e2, n, uv_lo, uv_hi):
        """(n + 1)^2 vertices, 2 n^2 triangles, normal e1 x e2 -> (vertexOffset, vertexCount, firstIndex, indexCount)"""
        vo, fi = sum(len(p) for p in pos), sum(len(i) for i in idx)
        s = np.arange(n + 1) / n
        a, b = np.meshgrid(s, s, indexing="xy")
        a, b = a.reshape(-1), b.reshape(-1)
        pos.append(np.asarray(p0, np.float64)[None] + a[:, None] * np.asarray(e1, np.float64)[None] + b[:, None] * np.asarray(e2, np.float64)[None])
        uv.append(np.stack([uv_lo[0] + (uv_hi[0] - uv_lo[0]) * a, uv_lo[1] + (uv_hi[1] - uv_lo[1]) * b], 1))
        tri = []
        for j in range(n):
            for i in range(n):
                v = j * (n + 1) + i
                tri += [v, v + 1, v + n + 2, v, v + n + 2, v + n + 1]
        idx.append(np.array(tri, np.uint32))
        return vo, (n + 1) ** 2, fi, len(tri)

    def node(geo, mat, matrix=eye4, kind=0):
        recs.append(geo + (M[mat],))
        nodes.append((len(recs) - 1, matrix))
        kinds.append(kind)

    node(grid((-8, -4, 0), (16, 0, 0), (0, 8, 0), 4, (0, 0), (1, 1)), "wall")
    uv_ranges = [((0.0, 0.0), (1.0, 1.0)), ((-0.5, -0.25), (2.5, 1.75)), ((0.125, 0.25), (0.875, 1.5))]
    for cx, cy, cards in columns():
        for k, (z, mat, (x0, x1), (y0, y1), facing) in enumerate(cards):
            lo, hi = uv_ranges[k % 3]
            if facing > 0:
                geo = grid((cx + x0, cy + y0, z), (x1 - x0, 0, 0), (0, y1 - y0, 0), 1, lo, hi)
            else:
                geo = grid((cx + x1, cy + y0, z), (x0 - x1, 0, 0), (0, y1 - y0, 0), 1, lo, hi)
            if isinstance(mat, tuple):   # a coincident pair: two prim-meshes over the same vertices and the same matrix, two materials
                node(geo, mat[0], kind=1)
                node(geo, mat[1], kind=1)
            else:
                node(geo, mat)
    cx, cy, cz = INSTANCED_AT
    geo = grid((cx - 1, cy - 1, cz), (2, 0, 0), (0, 2, 0), 2, (-0.25, 0.0), (1.25, 2.0))
    base = len(recs)
    recs.append(geo + (M["maskpot_ss"],))
    T = lambda t: gs.affine(np.eye(3), t).astype(np.float64)   # noqa: E731
    here = np.array(INSTANCED_AT)
    rotated = T(ROTATED_AT) @ gs.affine(gs.rot((1.0, 0.3, 0.2), 0.5) @ np.diag([1.1, 0.7, 1.6])).astype(np.float64) @ T(-here)
    mirrored = T(MIRRORED_AT) @ gs.affine(np.diag([-1.0, 1.0, 1.0])).astype(np.float64) @ T(-here)
    for mtx, kind in ((eye4, 2), (rotated.astype(np.float32), 2), (mirrored.astype(np.float32), 3)):
        nodes.append((base, mtx))
        kinds.append(kind)
    pos, uv, idx = np.concatenate(pos).astype(np.float32), np.concatenate(uv).astype(np.float32), np.concatenate(idx)
    nv = len(pos)
    uv[:, 1] = ((uv[:, 1].view(np.uint32) & np.uint32(0xFFFFFFFE)) | (np.arange(nv) % 2).astype(np.uint32)).view(np.float32)   # the handedness bit: HitTest reads the word as it is
    nrm, tan = np.tile((0.0, 0.0, 1.0), (nv, 1)), np.tile((1.0, 0.0, 0.0), (nv, 1))
    scene = dict(position=pos, normal_code=gs.encode_oct(nrm), tangent_code=gs.encode_oct(tan), texcoord=uv, color_code=np.full(nv, 0xFFFFFFFF, np.uint32),
                 indices=idx, records=np.array(recs, np.int32), node_record=np.array([r for r, _ in nodes], np.int32),
                 node_matrix=np.array([m for _, m in nodes], np.float32), node_kind=np.array(kinds, np.int8),   # 0 once, 1 coincident pair, 2 instanced, 3 instanced and mirrored
                 materials=materials(), material_names=np.array(MATERIALS))
    tex = textures()
    for t, (im, _) in enumerate(tex):
        scene[f"tex{t}"] = im
    scene["tex_sampler"] = np.array([s for _, s in tex], np.int32)
    return scene


# ---- world triangles (T1) and the flags ------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, scene, brk=None):
        rec9, inst, prim, cache = [], [], [], {}
        for n, (r, m) in enumerate(zip(scene["node_record"], scene["node_matrix"])):
            vo, _, fi, ni, _ = (int(x) for x in scene["records"][r])
            rows = [[float(x) for x in m[k]] for k in range(3)]
            for p in range(ni // 3):
                w = []
                for k in range(3):
                    v = vo + int(scene["indices"][fi + 3 * p + k])
                    key = (n if not np.array_equal(m, np.eye(4, dtype=np.float32)) else -1, v)
                    if key not in cache:
                        cache[key] = gt.xform_bits(rows, [float(x) for x in scene["position"][v]], 1)
                    w.append(cache[key])
                rec9.append(w[0] + [gt.fsub(w[1][k], w[0][k]) for k in range(3)] + [gt.fsub(w[2][k], w[0][k]) for k in range(3)])
                inst.append(n)
                prim.append(p)
        self.rec = np.array(rec9, np.float32)                       # p0 e1 e2: the nine record words
        self.inst, self.prim = np.array(inst), np.array(prim)
        self.pm = scene["node_record"][self.inst].astype(np.int64)  # instanceCustomIndex: the node's prim-mesh
        self.mat = np.maximum(scene["records"][self.pm][:, 4], 0)   # traceray_rq.glsl:39
        mt = scene["materials"][self.mat]
        self.mode, self.cutoff, self.tex = mt["alphaMode"], mt["alphaCutoff"], mt["pbrBaseColorTexture"]
        self.factor = mt["pbrBaseColorFactor"][:, 3]
        self.uvt = mt["uvTransform"][:, :8]
        self.nocull = mt["doubleSided"] == 1                         # accelstruct.cpp:148-149
        self.opaque = (self.mode == OPAQUE) | ((self.factor == 1.0) & (self.tex == -1) & (brk != "opaque_rule_no_arm"))   # :144-147
        det = np.linalg.det(scene["node_matrix"][:, :3, :3].astype(np.float64))
        self.flip = (det < 0)[self.inst] & (brk != "flip_ignored")
        self.kind = scene["node_kind"][self.inst]
        vo, fi = scene["records"][self.pm][:, 0].astype(np.int64), scene["records"][self.pm][:, 2].astype(np.int64)
        tri = scene["indices"][fi[:, None] + 3 * self.prim[:, None] + np.arange(3)[None]].astype(np.int64) + vo[:, None]
        self.uv = scene["texcoord"][tri]                             # (T, 3, 2) float32 words, handedness bit included
        w = self.rec.view(np.uint32)
        self.twin = np.full(len(w), -1)                              # the other triangle of a coincident pair: all nine words bit-identical
        for a in np.nonzero(self.kind == 1)[0]:
            same = np.nonzero((w == w[a]).all(1))[0]
            assert len(same) == 2
            self.twin[a] = same[same != a][0]


class VB:
    """gen_trace_kat's V for numpy arrays: a float64 value and the running bound of its fp32 evaluation"""
    __slots__ = ("v", "b")

    def __init__(self, v, b=0.0):
        self.v, self.b = v, b


def badd(a, b, sign=1.0):
    c, e = a.v + sign * b.v, a.b + b.b
    return VB(c, U * (np.abs(c) + e) + e)


def bmul(a, b):
    c = a.v * b.v
    e = np.abs(a.v) * b.b + np.abs(b.v) * a.b + a.b * b.b
    return VB(c, U * (np.abs(c) + e) + e + ETA)


def brecip(a):
    c = 1.0 / a.v
    e = a.b / (np.abs(a.v) * np.maximum(np.abs(a.v) - a.b, 1e-300))
    return VB(c, U * (np.abs(c) + e) + e + ETA)


def bcross(a, b):
    return [badd(bmul(a[1], b[2]), bmul(a[2], b[1]), -1.0), badd(bmul(a[2], b[0]), bmul(a[0], b[2]), -1.0), badd(bmul(a[0], b[1]), bmul(a[1], b[0]), -1.0)]


def bdot(a, b):
    return badd(badd(bmul(a[0], b[0]), bmul(a[1], b[1])), bmul(a[2], b[2]))


def t2(world, o, d, ft):
    """Moeller-Trumbore in the contract's tree for every (ray, triangle) -> det, t, u, v of type ft and, for float64, the bounds B(det), B(t), B(u), B(v), B(u + v)"""
    r = world.rec.astype(ft)
    p0, e1, e2 = [r[None, :, k] for k in range(3)], [r[None, :, 3 + k] for k in range(3)], [r[None, :, 6 + k] for k in range(3)]
    O, D = [o.astype(ft)[:, k, None] for k in range(3)], [d.astype(ft)[:, k, None] for k in range(3)]
    with np.errstate(all="ignore"):
        if ft is np.float64:
            V3 = lambda a: [VB(x) for x in a]  # noqa: E731
            tv = [badd(VB(O[k]), VB(p0[k]), -1.0) for k in range(3)]
            pv = bcross(V3(D), V3(e2))
            det = bdot(V3(e1), pv)
            qv = bcross(tv, V3(e1))
            inv = brecip(det)
            u, v, t = bmul(bdot(tv, pv), inv), bmul(bdot(V3(D), qv), inv), bmul(bdot(V3(e2), qv), inv)
            s = badd(u, v)
            grow = 1.0 + 2.0 ** -20
            return det.v, t.v, u.v, v.v, (det.b * grow, t.b * grow, u.b * grow, v.b * grow, s.b * grow)
        cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
        tv = [O[k] - p0[k] for k in range(3)]
        pv = cross(D, e2)
        det = dot(e1, pv)
        qv = cross(tv, e1)
        inv = ft(1) / det
        return det, dot(e2, qv) * inv, dot(tv, pv) * inv, dot(D, qv) * inv, None


# ---- opacity ---------------------------------------------------------------------------------------------------------------------------------------------
def opacity(scene, world, tri, u, v, bu, bv, ft, brk=None):
    """HitTest's opacity for candidate triangles `tri` hit at (u, v) -> (opacity of type ft, half-width of the interval the fp32 value lies in (float64 pass), decided,
    tag bits).  decided: a MASK cutoff outside the interval of the alpha, a NEAREST tap that names its texel"""
    n = len(tri)
    a = world.factor[tri].astype(ft)
    half, decided, tags = np.zeros(n), np.ones(n, bool), np.zeros(n, np.uint64)
    texid = world.tex[tri]
    for t in np.unique(texid[texid >= 0]):
        m = texid == t
        k = tri[m]
        img = scene[f"tex{t}"]
        h, w = img.shape[:2]
        mag, ws, wt = (int(x) for x in scene["tex_sampler"][t])
        uu, vv = u[m].astype(ft), v[m].astype(ft)
        b0 = (ft(1) - uu) - vv                                                            # traceray_rq.glsl:75
        uvs = world.uv[k].astype(ft)
        tc = uvs[:, 0] * b0[:, None] + uvs[:, 1] * uu[:, None] + uvs[:, 2] * vv[:, None]   # :79
        mt = world.uvt[k].astype(ft)
        x = tc[:, 0] * mt[:, 0] + tc[:, 1] * mt[:, 1] + mt[:, 2] + mt[:, 3]                # :82
        y = tc[:, 0] * mt[:, 4] + tc[:, 1] * mt[:, 5] + mt[:, 6] + mt[:, 7]
        lin = np.full(len(k), mag == tk.LINEAR)
        x0, x1, fa = tk.axis(x.astype(np.float64), w, np.full(len(k), ws), lin)[:3]
        y0, y1, fb = tk.axis(y.astype(np.float64), h, np.full(len(k), wt), lin)[:3]
        al = img[:, :, 3:4].astype(ft)
        ta = tk.blend(al[y0, x0], al[y0, x1], al[y1, x0], al[y1, x1], fa.astype(ft), fb.astype(ft))[:, 0] / ft(255)   # :84
        a[m] = a[m] * ta
        if ft is np.float64:
            au = np.abs(world.uv[k].astype(np.float64))
            e = au[:, 0] * (bu[m] + bv[m] + 2 * U)[:, None] + au[:, 1] * bu[m][:, None] + au[:, 2] * bv[m][:, None] + 8 * U * au.sum(1)
            am = np.abs(mt)
            ex = am[:, 0] * e[:, 0] + am[:, 1] * e[:, 1] + 8 * U * (np.abs(tc[:, 0] * mt[:, 0]) + np.abs(tc[:, 1] * mt[:, 1]) + am[:, 2] + am[:, 3])
            ey = am[:, 4] * e[:, 0] + am[:, 5] * e[:, 1] + 8 * U * (np.abs(tc[:, 0] * mt[:, 4]) + np.abs(tc[:, 1] * mt[:, 5]) + am[:, 6] + am[:, 7])
            xs, ys = np.abs(x * w), np.abs(y * h)
            if mag == tk.LINEAR:
                half[m] = np.abs(world.factor[k]) * (ex * w + ey * h + (xs + ys + 4) * tk.EPS)
            else:
                fx, fy = x * w - np.floor(x * w), y * h - np.floor(y * h)
                named = (np.minimum(fx, 1 - fx) > ex * w + xs * tk.EPS) & (np.minimum(fy, 1 - fy) > ey * h + ys * tk.EPS)
                half[m] = np.abs(world.factor[k]) * 4 * tk.EPS
                decided[m] &= named
            foot = np.stack([img[y0, x0, 3], img[y0, x1, 3], img[y1, x0, 3], img[y1, x1, 3]], 1).astype(np.int64)
            uniform = ((foot == 0).all(1) | (foot == 255).all(1))
            tg = np.zeros(len(k), np.uint64)
            if t == 2:
                tg |= np.where(uniform, TAG["MASK texel in a uniform block"], TAG["MASK texel in a mixed block"])
            if t == 3:
                tg |= TAG["general tap"]
            tg |= np.where(world.mat[k] == M["texrot"], TAG["uvTransform with rotation"], np.uint64(0))
            tags[m] = tg
    mask = world.mode[tri] == MASK
    cut = world.cutoff[tri].astype(ft)
    decided &= ~mask | (np.abs(a.astype(np.float64) - cut) > half) | (half == 0)
    over = (a >= cut) if brk == "mask_ge" else (a > cut)                                   # :88-91
    a = np.where(mask, np.where(over, ft(1), ft(0)), a)
    return a, np.where(mask, 0.0, half), decided, tags


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------------------
MASK32 = 0xFFFFFFFF


def draw(seed):
    """random.glsl pcg + rand on Python integers -> (state, the 23 mantissa bits: rand = m 2^-23 exactly)"""
    s = (seed * 747796405 + 2891336453) & MASK32
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & MASK32
    return s, ((w >> 22) ^ w) >> 9


@functools.lru_cache(None)
def zero_states(count=8):
    """the first `count` successor states, upward from 0, whose output is 0.0 -> seeds whose first, and whose second, draw is 0.0"""
    found, chunk, base = [], 1 << 22, 0
    while len(found) < count:
        s = np.arange(base, base + chunk, dtype=np.uint64)
        w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & np.uint64(MASK32)
        w = (w >> np.uint64(22)) ^ w
        found += [int(x) for x in s[(w >> np.uint64(9)) == 0]]
        base += chunk
        assert base < 1 << 32
    found = found[:count]
    inv = pow(747796405, -1, 1 << 32)
    back = lambda s: ((s - 2891336453) * inv) & MASK32  # noqa: E731
    first = [back(s) for s in found]
    second = [back(s) for s in first]
    for a, b in zip(first, second):
        assert draw(a)[1] == 0 and draw(draw(b)[0])[1] == 0 and draw(b)[1] != 0
    return first, second


# ---- rays ------------------------------------------------------------------------------------------------------------------------------------------------
def column_named(first_material):
    for cx, cy, cards in columns():
        if cards[0][1] == first_material:
            return cx, cy
    raise KeyError(first_material)


def build_rays(world):
    rng = np.random.default_rng(20261021)
    rec = world.rec.astype(np.float64)
    org, dirs, tmax, fam = [], [], [], []

    def interior(tris):
        b = rng.dirichlet((1, 1, 1), len(tris)) * 0.94 + 0.02
        return rec[tris, 0:3] + b[:, 1:2] * rec[tris, 3:6] + b[:, 2:3] * rec[tris, 6:9]

    def eyes(n):
        side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        return np.stack([rng.normal(0, 5, n), 2 + rng.normal(0, 4, n), side * (16 + rng.normal(0, 1.5, n))], 1)

    def emit(o, target, family, bounded=0.65):
        d = target - o
        dist = np.linalg.norm(d, axis=1)
        org.append(o); dirs.append(d / dist[:, None]); fam.append(np.full(len(o), family))
        tmax.append(np.where(rng.random(len(o)) < bounded, rng.uniform(0.2, 1.4, len(o)) * dist, INF))

    nt = len(rec)
    thin = np.nonzero((world.kind >= 2) | np.isin(world.mat, [M["masknpot"], M["maskrule"], M["opaquetex"]]))[0]   # the instanced mesh and the small cards: a third of the targets
    emit(eyes(1500), interior(np.where(rng.random(1500) < 0.33, thin[rng.integers(0, len(thin), 1500)], rng.integers(0, nt, 1500))), F_EYE)
    a, b = rng.integers(0, nt, 4000), rng.integers(0, nt, 4000)
    pa, pb = interior(a), interior(b)
    ok = np.abs(pa[:, 2] - pb[:, 2]) > 0.5                           # never inside a card's own plane
    pa, pb = pa[ok][:1100], pb[ok][:1100]
    emit(pa + (pb - pa) * 1e-5, pb, F_SURF)
    pairs = np.nonzero(world.kind == 1)[0]
    emit(eyes(600), interior(pairs[rng.integers(0, len(pairs), 600)]), F_PAIR)
    stair_cols = [(cx, cy) for cx, cy, cards in columns() if len(cards) >= 6 and cards[0][1] in ("zero", "zero_ss") and cards[1][1] == cards[0][1]]
    ns = 900
    pick = rng.integers(0, len(stair_cols), ns)
    edges = np.array(STEPS + (1.0,))
    lvl = rng.integers(0, 5, (ns, 2))                                 # every level of the stairs alike, whatever its width
    tgt = np.array(stair_cols)[pick] + edges[lvl] + rng.uniform(0.02, 0.98, (ns, 2)) * (edges[lvl + 1] - edges[lvl])
    e = eyes(ns)
    e[:, :2] = tgt + (e[:, :2] - tgt) * 0.05                          # steep: the ray stays inside its column's footprint
    emit(e, np.concatenate([tgt, np.zeros((ns, 1))], 1), F_STAIR)
    org, dirs, tmax, fam = np.concatenate(org), np.concatenate(dirs), np.concatenate(tmax), np.concatenate(fam)
    seeds = tk.words(len(org), 3200).astype(np.int64)

    # exact rows: axis-parallel rays from dyadic origins onto cards at integer depths; the distance to the nearest card that faces the ray is exact
    ex_o, ex_d = [], []
    for cx, cy in (column_named("zero"), column_named("zero_ss"), (COLS_X[3], ROW_IN[0]), (COLS_X[4], ROW_IN[0])):
        for dx, dy in zip(EXACT_DX, EXACT_DY):
            for sgn in (1.0, -1.0):
                ex_o.append((cx + dx, cy + dy, sgn * 8.0)); ex_d.append((0.0, 0.0, -sgn))
    ex_o, ex_d = np.array(ex_o), np.array(ex_d)
    return dict(org=org, dirs=dirs, tmax=tmax, fam=fam, seeds=seeds, exact_org=ex_o, exact_dir=ex_d)


# ---- the walk --------------------------------------------------------------------------------------------------------------------------------------------
class Result:
    pass


def evaluate(scene, world, org, dirs, tmax, seeds, ft, brk=None):
    """the model on every ray in type ft.  Returns a Result of arrays: the sorted key list, closest (T5), shadow (T6), the any-hit-off forms, decisions, and for
    float64 the margins and tags"""
    n = len(org)
    o32, d32 = org.astype(np.float32), dirs.astype(np.float32)
    det, t, u, v, bounds = t2(world, o32, d32, ft)
    with np.errstate(all="ignore"):
        front = np.where(world.flip[None], det < 0, det > 0)
        facing = world.nocull[None] | front
        inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (det != 0)
        acc = facing & inside & (t > 0)
        tt = np.where(acc, t, np.inf).astype(np.float64)
    if brk == "tie_desc":
        order = np.argsort(tt[:, ::-1], 1, kind="stable")
        order = tt.shape[1] - 1 - order
    else:
        order = np.argsort(tt, 1, kind="stable")            # equal t: the lower world index first
    nk = acc.sum(1)
    K = max(int(nk.max()), KEYS)
    order = order[:, :K]
    rows = np.arange(n)[:, None]
    kt = np.where(np.arange(K)[None] < nk[:, None], tt[rows, order], np.inf)
    kw = np.where(np.isfinite(kt), order, -1)
    ku, kv = u[rows, order], v[rows, order]
    R = Result()
    R.nk, R.kw, R.kt, R.ku, R.kv = nk, kw, kt, ku, kv
    # opacity of every non-opaque key
    flat = np.nonzero((kw >= 0) & ~world.opaque[np.maximum(kw, 0)])
    tri = kw[flat]
    if bounds is not None:
        bdet, bt, bu_, bv_, _ = bounds
        kbt, kbu, kbv = bt[rows, order], bu_[rows, order], bv_[rows, order]
        R.kbt, R.kbu, R.kbv = kbt, kbu, kbv
        fbu, fbv = kbu[flat], kbv[flat]
    else:
        fbu = fbv = np.zeros(len(tri))
    op, half, decided, otag = opacity(scene, world, tri, ku[flat], kv[flat], fbu, fbv, ft, brk)
    kop, khalf, kdec, ktag = np.full((n, K), 2.0), np.zeros((n, K)), np.ones((n, K), bool), np.zeros((n, K), np.uint64)
    kop[flat], khalf[flat], kdec[flat], ktag[flat] = op.astype(np.float64), half, decided, otag
    kopaque = (kw >= 0) & world.opaque[np.maximum(kw, 0)]
    lim = tmax.astype(np.float32).astype(np.float64)
    bounded = lim < 1e30

    def walk(r, shadow):
        """-> (commit position or -1, seed afterwards, draws, every comparison decided, the 0.0 draw that committed a zero-opacity candidate / the certain hit)"""
        s, draws, ok, zero_commit, zero_certain, frac = int(seeds[r]), 0, True, False, False, False
        for c in range(int(nk[r])):
            if shadow and not (kt[r, c] <= lim[r] if brk == "tmax_inclusive" else kt[r, c] < lim[r]):
                break
            if kopaque[r, c]:
                if brk == "opaque_draws":
                    s, _ = draw(s); draws += 1
                return c, s, draws, ok, zero_commit, zero_certain, frac
            a, h = kop[r, c], khalf[r, c]
            if brk == "count_excludes_ties" and a <= 0 and c + 1 < nk[r] and kt[r, c + 1] == kt[r, c] and (kopaque[r, c + 1] or kop[r, c + 1] >= 1):
                continue   # (the zero-opacity candidate that ties with the hit is not counted: no draw)
            s, m = draw(s)
            draws += 1
            x = m * 2.0 ** -23
            ok &= bool(kdec[r, c]) and (h == 0 or x < a - h or x > a + h)
            frac |= 0 < a < 1
            rejected = (x >= a) if brk == "reject_ge" else (x > a)       # traceray_rq.glsl:98
            if brk == "zero_never_commits" and a <= 0:
                rejected = True
            if not rejected:
                zero_commit, zero_certain = (m == 0 and a <= 0), (m == 0 and a >= 1 - 1e-6)
                return c, s, draws, ok, zero_commit, zero_certain, frac
        return -1, s, draws, ok, zero_commit, zero_certain, frac

    R.c_pos, R.c_seed, R.c_draws = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    R.s_hit, R.s_seed, R.s_draws = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64)
    R.ok, R.tags = np.ones(n, bool), np.zeros(n, np.uint64)
    for r in range(n):
        c, s, dr, ok, zc, zh, frac = walk(r, False)
        R.c_pos[r], R.c_seed[r], R.c_draws[r] = c, s, dr
        c2, s2, dr2, ok2, zc2, zh2, _ = walk(r, True)
        R.s_hit[r], R.s_seed[r], R.s_draws[r] = c2 >= 0, s2, dr2
        R.ok[r] = ok and ok2
        if ft is np.float64:
            tg = np.uint64(0)
            end = c if c >= 0 else int(nk[r])
            zero = [(not kopaque[r, k]) and kop[r, k] <= 0 for k in range(int(nk[r]))]
            nf, nb = sum(zero[:end]), sum(zero[end + 1:])
            tg |= TAG[TAGS[min(nf, 4)]]
            if c >= 0:
                tg |= TAG[TAGS[5 + min(nb, 4)]]
                if nf and nb:
                    tg |= TAG["zero on both sides of the hit"]
                w = int(kw[r, c])
                tg |= TAG["BLAS instance committed"] if world.kind[w] >= 2 else TAG["merged structure committed"]
                if world.opaque[w] and world.mode[w] != OPAQUE or world.mat[w] == M["opaquetex"]:
                    tg |= TAG["opaque by rule"]
            else:
                tg |= TAG["miss"]
            for k in range(min(end + 1, int(nk[r])) - 1):   # ties among the keys walked: (k, k + 1) twins
                if world.twin[int(kw[r, k])] == kw[r, k + 1]:
                    a, b = int(kw[r, k]), int(kw[r, k + 1])
                    za, zb = (not world.opaque[a]) and kop[r, k] <= 0, (not world.opaque[b]) and kop[r, k + 1] <= 0
                    name = "tie (zero, zero)" if za and zb else "tie (zero, opaque)" if za and world.opaque[b] else "tie (fractional, fractional)" if not (za or zb or world.opaque[a] or world.opaque[b]) else None
                    if name:
                        tg |= TAG[name]
            if c >= 0 and world.twin[int(kw[r, c])] >= 0 and c + 1 < nk[r] and kw[r, c + 1] == world.twin[int(kw[r, c])]:   # the lower index committed, its twin is never walked
                if world.opaque[int(kw[r, c])]:
                    tg |= TAG["tie (opaque, zero)"]
                elif 0 < kop[r, c] < 1:
                    tg |= TAG["tie (fractional, fractional)"]
            if frac:
                tg |= TAG["fractional candidate walked"]
            for k in range(min(end + 1, int(nk[r]))):
                tg |= ktag[r, k]
            if bounded[r] and (kt[r, :int(nk[r])] >= lim[r]).any() and not R.s_hit[r]:
                tg |= TAG["shadow ray ended by tmax"]
            if dr2:
                tg |= TAG["shadow draws (RTX differs)"]
            if zc:
                tg |= TAG["0.0 on a zero-opacity candidate, closest"]
            if zc2:
                tg |= TAG["0.0 on a zero-opacity candidate, shadow"]
            if zh or zh2:
                tg |= TAG["0.0 on the certain hit's own draw"]
            R.tags[r] = tg
    R.s_seed_rtx = R.s_seed.copy() if brk == "rtx_seed_written" else seeds.copy()
    # any-hit off: every triangle opaque
    R.a_pos = np.where(nk > 0, 0, -1)
    with np.errstate(invalid="ignore"):
        R.a_shadow = (kt[:, 0] <= lim) if brk == "tmax_inclusive" else (kt[:, 0] < lim)
    # decisions: what the float32 and the float64 evaluation must take alike
    R.decisions = [nk, kw[:, :K], R.c_pos, R.c_seed, R.s_hit, R.s_seed, R.a_shadow]
    if ft is np.float64:
        with np.errstate(all="ignore"):
            mirrored = (world.kind == 3)[None] & inside & (t > 0)
            R.tags |= np.where((mirrored & ~facing).any(1), TAG["mirrored instance culled"], np.uint64(0))
            R.tags |= np.where((mirrored & facing).any(1), TAG["mirrored instance accepted"], np.uint64(0))
            mn = np.minimum(np.minimum(u, v), (1 - u) - v)
            limx = np.where(bounded, lim, np.inf)[:, None]
            reach = facing & (t > -TZERO) & (t < limx * (1 + SEP) + SEP)
            unsafe = (reach & (np.abs(mn) < EDGE)).any(1)
            unsafe |= (reach & (mn > -EDGE) & ~(np.abs(det) > 2 * bdet)).any(1)
            unsafe |= (facing & (mn > -EDGE) & (np.abs(t) < TZERO)).any(1)
            near_end = (facing & (mn > -EDGE) & (np.abs(t - limx) < SEP * np.maximum(1.0, limx))).any(1)
            gap = kt[:, 1:] - kt[:, :-1]
            tied = (world.twin[np.maximum(kw[:, :-1], 0)] == kw[:, 1:]) & (kw[:, 1:] >= 0)
            close = np.isfinite(kt[:, 1:]) & (gap < SEP * np.maximum(1.0, kt[:, :-1])) & ~tied
            unsafe |= close.any(1)
        R.safe, R.near_end = ~unsafe, near_end
    return R


def mint(brk=None, verbose=False):
    scene = build_scene()
    world = World(scene, brk)
    assert len(world.rec) <= 300
    rays = build_rays(world)
    first, second = zero_states()
    org, dirs, tmax, fam, seeds = rays["org"], rays["dirs"], rays["tmax"], rays["fam"], rays["seeds"]
    exact_kind = np.zeros(len(org), np.int8)

    # exact rows: their own t from an unbounded evaluation of the any-hit-off form, then the three bounds
    plain = World(scene)
    E = evaluate(scene, plain, rays["exact_org"], rays["exact_dir"], np.full(len(rays["exact_org"]), INF), np.zeros(len(rays["exact_org"]), np.int64), np.float64)
    assert (E.nk > 0).all()
    t0 = E.kt[:, 0].astype(np.float32)
    assert (t0.astype(np.float64) == E.kt[:, 0]).all()
    ne = len(t0)
    eo, ed = np.tile(rays["exact_org"], (3, 1)), np.tile(rays["exact_dir"], (3, 1))
    et = np.concatenate([t0, np.nextafter(t0, np.float32(np.inf)), np.where(np.arange(ne) % 2 == 0, 0.0, -1.0).astype(np.float32)])
    ek = np.repeat([1, 2, 3], ne).astype(np.int8)
    es = tk.words(3 * ne, 3201).astype(np.int64)

    # zero-draw rays: exact rows with chosen seeds
    cz, cf, cc = column_named("zero"), (COLS_X[2], ROW_IN[0]), (COLS_X[3], ROW_IN[0])
    zo, zd, zs, zt = [], [], [], []
    for k in range(8):
        a, b = first[k], second[k]
        dy = EXACT_DY[k % 4]
        for (cx, cy), dx, seed in ((cz, (0.125, 0.625)[k % 2], a), (cz, (0.125, 0.625)[k % 2], b), (cf, (0.125, 0.625)[k % 2], a), (cf, (0.125, 0.625)[k % 2], b),
                                   (cc, (-0.625, -0.375)[k % 2], a), (cc, (0.125, 0.625)[k % 2], b)):
            for bound in (INF, 7.5):   # 7.5: past every card in front of the wall (|z| <= 5 from z = 8 is t <= 7), in front of the wall (t = 8)
                zo.append((cx + dx, cy + dy, 8.0)); zd.append((0.0, 0.0, -1.0)); zs.append(seed); zt.append(bound)
        for (cx, cy), dx, seed in ((cc, (0.125, -0.375)[k % 2], a),):   # from behind: the MASK card of opacity 1 is the certain hit, its own draw is 0.0
            for bound in (INF, 7.5):
                zo.append((cx + dx, cy + dy, -8.0)); zd.append((0.0, 0.0, 1.0)); zs.append(seed); zt.append(bound)
    zo, zd, zs, zt = np.array(zo), np.array(zd), np.array(zs, np.int64), np.array(zt)
    nz = len(zo)

    # the order: ordinary rays; indices 128 .. 191 hold zero-draw rays only (one whole wavefront of 64 lanes); the other zero-draw rays and the exact rows
    # are spread among ordinary rays from index 200 on, all inside the first 4097
    n_ord = len(org)
    block = np.arange(nz)[:64] if nz >= 64 else np.resize(np.arange(nz), 64)
    rest = np.arange(nz)
    sp_o = np.concatenate([zo[rest], eo]); sp_d = np.concatenate([zd[rest], ed]); sp_t = np.concatenate([zt[rest], et]); sp_s = np.concatenate([zs[rest], es])
    sp_f = np.concatenate([np.full(len(rest), F_ZERO), np.full(len(eo), F_EXACT)]); sp_k = np.concatenate([np.zeros(len(rest), np.int8), ek])
    slots = 200 + 16 * np.arange(len(sp_o))
    assert slots[-1] < 4097
    total = n_ord + 64 + len(sp_o)
    assert total > 4097
    O, D, T, S, Fm, Kd = np.zeros((total, 3)), np.zeros((total, 3)), np.zeros(total), np.zeros(total, np.int64), np.zeros(total, np.int64), np.zeros(total, np.int8)
    where = np.full(total, -1)
    where[128:192] = -2
    where[slots] = -3
    O[128:192], D[128:192], T[128:192], S[128:192], Fm[128:192] = zo[block], zd[block], zt[block], zs[block], F_ZERO
    O[slots], D[slots], T[slots], S[slots], Fm[slots], Kd[slots] = sp_o, sp_d, sp_t, sp_s, sp_f, sp_k
    free = where == -1
    assert free.sum() == n_ord
    O[free], D[free], T[free], S[free], Fm[free] = org, dirs, tmax, seeds, fam
    org, dirs, tmax, seeds, fam, exact_kind = O.astype(np.float32), D.astype(np.float32), T.astype(np.float32), S, Fm, Kd

    R64 = evaluate(scene, world, org, dirs, tmax, seeds, np.float64, brk)
    R32 = evaluate(scene, world, org, dirs, tmax, seeds, np.float32, brk) if brk is None else R64   # (a broken model is only compared with the fixture: its kept mask is never used)
    same = np.ones(len(org), bool)
    for a, b in zip(R64.decisions, R32.decisions):
        k = min(a.shape[1], b.shape[1]) if a.ndim == 2 else None
        same &= (a[:, :k] == b[:, :k]).all(1) if a.ndim == 2 else (a == b)
    special = (fam == F_EXACT) | (fam == F_ZERO)
    kept = same & R64.ok & R32.ok & R64.safe & (~R64.near_end | special)
    if brk is None:
        assert kept[special].all(), ("an exact row or a zero-draw ray fails a rule other than the margin to tmax", np.nonzero(special & ~kept)[0][:8])
        check_exact(world, org, dirs, R64, special)
    tags = R64.tags.copy()
    for k, name in ((1, "exact row: tmax = t"), (2, "exact row: tmax = nextafter(t)"), (3, "exact row: tmax <= 0")):
        tags[exact_kind == k] |= TAG[name]
    if brk is None:
        assert not R64.a_shadow[exact_kind == 1].any() and R64.a_shadow[exact_kind == 2].all() and not R64.a_shadow[exact_kind == 3].any()   # exclusive; hit; empty

    pos = np.maximum(R64.c_pos, 0)
    rows = np.arange(len(org))
    hit = R64.c_pos >= 0
    cw = np.where(hit, R64.kw[rows, pos], -1)
    aw = R64.kw[:, 0]
    out = dict(scene)
    out.update(
        ray_origin=org, ray_direction=dirs, ray_tmax=tmax, ray_seed=seeds.astype(np.uint32), ray_family=fam.astype(np.uint8), ray_exact=exact_kind,
        kept=kept, tags=tags, tag_names=np.array(TAGS), family_names=np.array(FAMILIES),
        world_inst=world.inst.astype(np.int32), world_prim=world.prim.astype(np.int32), world_pm=world.pm.astype(np.int32), world_rec=world.rec,
        key_world=R64.kw[:, :KEYS].astype(np.int32), key_t=np.where(np.isfinite(R64.kt[:, :KEYS]), R64.kt[:, :KEYS], 0.0),
        key_bt=np.where(R64.kw[:, :KEYS] >= 0, R64.kbt[:, :KEYS], 0).astype(np.float32), key_count=R64.nk.astype(np.int32),
        closest_world=cw.astype(np.int32), closest_tuv=np.where(hit[:, None], np.stack([R64.kt[rows, pos], R64.ku[rows, pos], R64.kv[rows, pos]], 1), 0.0),
        closest_bound=np.where(hit[:, None], np.stack([R64.kbt[rows, pos], R64.kbu[rows, pos], R64.kbv[rows, pos]], 1), 0.0).astype(np.float32),
        closest_seed=R64.c_seed.astype(np.uint32), closest_draws=R64.c_draws.astype(np.int32),
        shadow_hit=R64.s_hit, shadow_seed=R64.s_seed.astype(np.uint32), shadow_seed_rtx=R64.s_seed_rtx.astype(np.uint32), shadow_draws=R64.s_draws.astype(np.int32),
        opaque_world=aw.astype(np.int32), opaque_tuv=np.where((aw >= 0)[:, None], np.stack([R64.kt[:, 0], R64.ku[:, 0], R64.kv[:, 0]], 1), 0.0),
        opaque_bound=np.where((aw >= 0)[:, None], np.stack([R64.kbt[:, 0], R64.kbu[:, 0], R64.kbv[:, 0]], 1), 0.0).astype(np.float32), opaque_shadow=R64.a_shadow)
    return out


def check_exact(world, org, dirs, R, special):
    """every T2 operation on every candidate an exact row or a zero-draw ray meets is exact in fp32: gen_trace_kat.t2_truth in fractions.Fraction"""
    for r in np.nonzero(special)[0]:
        for c in range(int(R.nk[r])):
            w = int(R.kw[r, c])
            row = np.concatenate([world.rec[w], [0.0], org[r], dirs[r]]).astype(np.float64)
            _, _, tuv, _, exact_ops = gt.t2_truth(row)
            assert exact_ops and float(tuv[0]) == R.kt[r, c] and float(tuv[1]) == R.ku[r, c] and float(tuv[2]) == R.kv[r, c], (r, c)


def check_caps(out, report=False):
    kept, fam, tags = out["kept"], out["ray_family"], out["tags"]
    drops = {FAMILIES[f]: 1.0 - kept[fam == f].mean() for f in range(len(FAMILIES))}
    counts = {name: int(((tags[kept] & TAG[name]) != 0).sum()) for name in TAGS}
    if report:
        print("rays", len(kept), "triangles", len(out["world_rec"]))
        print("dropped per family: " + ", ".join(f"{k} {v:.1%}" for k, v in drops.items()))
        print("kept rays per tag: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    over = [f"{k}: {v:.1%}" for k, v in drops.items() if v > 0.10]
    assert not over, "ray families with more than 10 % dropped: " + "; ".join(over)
    short = [f"{k}: {v}" for k, v in counts.items() if v < (4 if k in SMALL_TAGS else 50)]
    assert not short, "tags with too few kept rays: " + "; ".join(short)
    return drops, counts


def main(path=None, brk=None, caps=True):
    assert brk is None or brk in BREAK
    out = mint(brk)
    if caps:
        check_caps(out, report=True)
    path = path or OUT
    gs.write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(*sys.argv[1:3])

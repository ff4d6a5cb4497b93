"""The exact model of the intersection arithmetic (vk_raytrace_amd/csrc/pt_trace.h) and its fixture, tests/golden/trace_kat.npz.

    python tests/golden/gen_trace_kat.py        # seeded, deterministic: the file regenerates byte for byte

Written from DESIGN.md section 3 and from the comments that state each function's promise, not from the code.  fp32 inputs are rationals, so truth is computed
with fractions.Fraction and carries no rounding at all; where a result must be an fp32 number (T1, the transformed ray of enter_instance) every operation is
rounded from the exact rational with integers, to nearest even (rnd).  tests/trace_kat_io.py packs the rows and holds the assertions; tests/test_trace_model.py
and tests/test_trace_gpu.py run them on the host build, the oracle and the device.

T1 (bit model).  p_i = ((M.c0 x + M.c1 y) + M.c2 z) + M.c3, every product and sum rounded once, then e1 = p1 - p0, e2 = p2 - p0 rounded once.  Zeros carry the
IEEE sign: a product's is the xor of its factors', an exact sum is +0 unless both terms are -0.

T2 (truth and a derived bound).  Exact det, u, v, t of Moeller-Trumbore on (p0, e1, e2, o, d).  The bound follows the contract's expression tree
tv = o - p0, pv = d x e2, det = e1 . pv, qv = tv x e1, nu = tv . pv, nv = d . qv, nt = e2 . qv, inv = 1 / det, u = nu inv, v = nv inv, t = nt inv, s = u + v
with cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x) and dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  With x^ the computed and x the
exact value of a node, B(x) >= |x^ - x|, unit roundoff u = 2^-24 and eta = 2^-149 for a product that may underflow:
    input       B = 0
    c = a +- b  E = B(a) + B(b)                                  B(c) = u (|c| + E) + E
    c = a b     E = |a| B(b) + |b| B(a) + B(a) B(b)              B(c) = u (|c| + E) + E + eta
    c = 1 / a   E = B(a) / (|a| (|a| - B(a))),  |a| > B(a)       B(c) = u (|c| + E) + E + eta
(the computed operands lie within B of the exact ones, the exact operation moves by at most E, the rounding adds u times the magnitude of what is rounded).
Every quantity on the right is exact, so the bound is derived from the inputs alone; nothing is measured.  A row is DECIDED when |det| > 2 B(det) and each of
u, v, 1 - u - v is farther from 0 than its bound (B(u), B(v), B(s)); then the signs of det^, u^, v^ and 1 - s^ are the exact ones, u^ <= 1 follows, and the
fp32 verdict must be the exact verdict.  The fixture stores t, u, v as float64 (relative error 2^-53) and the bounds as float32 rounded up after a factor
1 + 2^-20, which covers both.
Lattice rows are rows on which every operation of the tree is exact (each intermediate is an fp32 number, checked here): verdict and t, u, v are asserted bit
for bit, which pins the inclusive edges u == 0, v == 0, u + v == 1 (accepted), u == 1 at vertex 1, and det == 0 (rejected).

The box tests.  Truth: the exact interval of t with o + t d inside the box and 0 <= t <= lim, for the true d; a zero component constrains the origin only.
One-sided promise: interval non-empty => the child is reported (both node forms).  Tightness: a reported child has a non-empty exact interval, with lim grown
to lim (1 + REL), against the box grown per axis by g_a.  Derivation of g_a from the stated constants (make_raybox, wide_node_step):
  * n = -(o idir) is biased by 2^-21 |o idir| towards "hit"; o idir, the negation's sum and the bias carry three roundings, so the plane moves outwards by at most
    (2^-21 + 2^-23) (1 + 2u) |o_a| in space: BETA = 1.26 x 2^-21.
  * the decision multiplies the near end by 0.9999996f = 1 - 7 x 2^-24 and the far end by 1.0000004f = 1 + 3 x 2^-23, "4e-7 relative on both ends"; idir = fl(1 / d),
    the plane's FMA and that product add 2^-24 each: a relative error of at most 4.2e-7 + 3 x 6e-8 < REL = 6.6e-7 of the distance T d_a travelled along the axis.  A
    point inside the grown slab has |T d_a| <= (|o_a| (1 + BETA) + M_a) / (1 - REL), M_a = max(|lo_a|, |hi_a|), and REL was rounded up to cover those factors.
  * |d_a| < 1e-18 is replaced by 1e-18: over T <= (|o_m| + M_m) (1 + 1e-5) / |d_m| (m the axis of the largest |d|) the point moves by at most CLAMP_a = 1e-18 x that.
      g_a = BETA |o_a| + REL (|o_a| + M_a) + CLAMP_a
  Compact nodes (cnode_visit): the decoded plane lies within one grid step 2^(e-127) outside the fp32 plane (e the smallest exponent >= 27 whose 2047 steps cover the
  extent of the node's real children on that axis, origin p_a their lowest plane); b = p idir + n is biased by 8e-7 (|b| + 2047 |s|), i.e. in space by
  8e-7 (|p_a - o_a| + BETA |o_a| + 2047 step_a) and four more roundings: CB = 8.3e-7.
      g_a(compact) = step_a + BETA |o_a| + CB (|p_a - o_a| + BETA |o_a| + 2047 step_a) + REL (|o_a| + M_a + step_a) + CLAMP_a
  These margins are derived, not fitted; a violation is a finding, not a reason to widen them.
Order of a visit (comment on wide_node_step): the children reported are exactly the hit set, all but the nearest pushed farthest first, the nearest returned.  The
model knows a child's entry distance only up to the margins: it lies between the entry into the grown box times (1 - REL) and the entry into the exact box.  A
sequence is wrong when a child that must be farther comes after one that must be nearer; ties, and everything inside the margins, may fall either way.

enter_instance: o' = W (o, 1), d' = W (d, 0) in T1's order (bit model, stored), then make_raybox(o', d') widened by eps |idir|, eps = padC1 max|o| + padC0 (stored
exactly rounded to float64); tests/trace_kat_io.py compares within the fp32 rounding of that expression.

Domain: |coordinates| < 2^20, directions with a component of ordinary size (the promise "a ray moves < 1 ulp along a clamped axis" needs a bounded T).  The
degenerate sets (Inf, NaN, denormal and repeated vertices; planes and origins up to 1e30) are outside it: leg-to-leg bits only.
"""
import math
import os
import sys
from fractions import Fraction as Fr

import numpy as np

BVH_LEAF, BVH_ALPHA, BVH_NONE = 0x80000000, 0x40000000, 0xFFFFFFFF
TRI_NOCULL, TRI_FLIP = 2, 4
FLT_MAX = float(np.finfo(np.float32).max)
U, ETA = Fr(1, 1 << 24), Fr(1, 1 << 149)
BETA = Fr(126, 100) / (1 << 21)
REL = Fr(66, 10 ** 8)
CB = Fr(83, 10 ** 8)
CLAMP_D = Fr(float(np.float32(1e-18)))
GRID = 2047
SETS = ("interior", "miss", "sliver", "flags", "lattice")
LATTICE_CATEGORIES = ("vertex0", "vertex1 (u == 1)", "vertex2", "u == 0", "v == 0", "u + v == 1", "interior", "outside", "t < 0", "det == 0 in the plane",
                      "det == 0 along an edge")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trace_kat.npz")


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------------------------------
def rnd(q):
    """the fp32 number nearest to the rational q, ties to even, as a Fraction; integers only"""
    if q == 0:
        return Fr(0)
    s, q = (-1, -q) if q < 0 else (1, q)
    n, d = q.numerator, q.denominator
    e = n.bit_length() - d.bit_length()
    if (n < (d << e)) if e >= 0 else ((n << -e) < d):
        e -= 1  # 2^e <= q < 2^(e + 1)
    k = max(e, -126) - 23  # the quantum
    a, b = (n << -k, d) if k < 0 else (n, d << k)
    m, r = divmod(a, b)
    if 2 * r > b or (2 * r == b and (m & 1)):
        m += 1
    v = Fr(m << k) if k >= 0 else Fr(m, 1 << -k)
    if v >= Fr(1 << 128):
        raise OverflowError("outside the domain")
    return s * v


def fr(x):
    return Fr(float(x))


def neg(x):
    return math.copysign(1.0, x) < 0


def fmul(a, b):
    r = float(rnd(fr(a) * fr(b)))
    return math.copysign(0.0, -1.0 if neg(a) != neg(b) else 1.0) if r == 0 else r


def fadd(a, b):
    q = fr(a) + fr(b)
    if q == 0:
        return -0.0 if (neg(a) and neg(b)) else 0.0
    return float(rnd(q))


def fsub(a, b):
    return fadd(a, -b)


def xform_bits(rows, p, w):
    """rows: three (x, y, z, w) rows of a 3 x 4 matrix.  ((r.x p.x + r.y p.y) + r.z p.z) + r.w w for w = 1, without the last term for w = 0"""
    out = []
    for r in rows:
        s = fadd(fadd(fmul(r[0], p[0]), fmul(r[1], p[1])), fmul(r[2], p[2]))
        out.append(fadd(s, float(r[3])) if w else s)
    return out


class V:
    __slots__ = ("v", "b")

    def __init__(self, v, b=Fr(0)):
        self.v, self.b = v, b


def vadd(a, b, sign=1):
    c, e = a.v + sign * b.v, a.b + b.b
    return V(c, U * (abs(c) + e) + e)


def vmul(a, b):
    c = a.v * b.v
    e = abs(a.v) * b.b + abs(b.v) * a.b + a.b * b.b
    return V(c, U * (abs(c) + e) + e + ETA)


def vrecip(a):
    c = 1 / a.v
    e = a.b / (abs(a.v) * (abs(a.v) - a.b))
    return V(c, U * (abs(c) + e) + e + ETA)


def vcross(a, b):
    return [vadd(vmul(a[1], b[2]), vmul(a[2], b[1]), -1), vadd(vmul(a[2], b[0]), vmul(a[0], b[2]), -1), vadd(vmul(a[0], b[1]), vmul(a[1], b[0]), -1)]


def vdot(a, b):
    return vadd(vadd(vmul(a[0], b[0]), vmul(a[1], b[1])), vmul(a[2], b[2]))


def t2_truth(row):
    """row: p0 e1 e2 flags o d (16 numbers).  Returns verdict, decided, (t, u, v) exact or None, their bounds, and whether every operation was exact"""
    f = [V(fr(x)) for x in row]
    p0, e1, e2, o, d = f[0:3], f[3:6], f[6:9], f[10:13], f[13:16]
    flags = int(row[9])
    nodes = []

    def keep(x):
        nodes.extend(x if isinstance(x, list) else [x])
        return x
    pv = keep(vcross(d, e2))
    det = keep(vdot(e1, pv))
    exact_ops = all(rnd(x.v) == x.v for x in nodes) and all(rnd(d[i].v * e2[j].v) == d[i].v * e2[j].v for i in range(3) for j in range(3) if i != j) \
        and all(rnd(e1[i].v * pv[i].v) == e1[i].v * pv[i].v for i in range(3)) and rnd(e1[0].v * pv[0].v + e1[1].v * pv[1].v) == e1[0].v * pv[0].v + e1[1].v * pv[1].v
    if det.v == 0:
        return False, False, None, None, exact_ops
    tv = [vadd(o[k], p0[k], -1) for k in range(3)]
    qv = vcross(tv, e1)
    nu, nv, nt = vdot(tv, pv), vdot(d, qv), vdot(e2, qv)
    front = (det.v < 0) if (flags & TRI_FLIP) else (det.v > 0)
    u_, v_, t_ = nu.v / det.v, nv.v / det.v, nt.v / det.v
    verdict = ((flags & TRI_NOCULL) != 0 or front) and 0 <= u_ <= 1 and v_ >= 0 and u_ + v_ <= 1
    if exact_ops:  # the remaining operations, products and partial sums included
        vals = [x.v for x in tv + qv + [nu, nv, nt]] + [1 / det.v, u_, v_, t_, u_ + v_]
        for a, b in ((tv, pv), (d, qv), (e2, qv)):
            vals += [a[i].v * b[i].v for i in range(3)] + [a[0].v * b[0].v + a[1].v * b[1].v]
        vals += [tv[i].v * e1[j].v for i in range(3) for j in range(3) if i != j]
        exact_ops = all(rnd(x) == x for x in vals)
    if not abs(det.v) > 2 * det.b:
        return verdict, False, (t_, u_, v_), None, exact_ops
    inv = vrecip(det)
    u, v, t = vmul(nu, inv), vmul(nv, inv), vmul(nt, inv)
    s = vadd(u, v)
    decided = abs(u.v) > u.b and abs(v.v) > v.b and abs(1 - s.v) > s.b
    return verdict, decided, (t_, u_, v_), (t.b, u.b, v.b), exact_ops


def up32(q):
    """a float32 no smaller than q (1 + 2^-20)"""
    x = np.float32(float(q * (1 + Fr(1, 1 << 20))))
    return x if fr(x) >= q else np.nextafter(x, np.float32(np.inf))


# ---- triangles -------------------------------------------------------------------------------------------------------------------------------------------
def unit(rng, n=None):
    v = rng.normal(size=3 if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_triangle(rng, sliver=False):
    s = 10.0 ** rng.uniform(-2, 2)
    p0, e1, e2 = s * rng.normal(size=3), s * rng.normal(size=3), s * rng.normal(size=3)
    if sliver:  # the third vertex within 1e-3 of the opposite edge (in units of that edge)
        e2 = rng.uniform(0.05, 0.95) * e1 + 1e-3 * rng.uniform(0.05, 1.0) * np.linalg.norm(e1) * unit(rng)
    if rng.random() < 0.3:
        p0 = p0 + 10.0 ** rng.uniform(1, 3.7) * unit(rng)
    return p0.astype(np.float32), e1.astype(np.float32), e2.astype(np.float32)


def aimed_row(rng, tri, inside, flags):
    p0, e1, e2 = (x.astype(np.float64) for x in tri)
    if inside:
        r1, r2 = math.sqrt(rng.random()), rng.random()
        a, b = r1 * (1 - r2), r1 * r2
    else:
        while True:
            a, b = rng.uniform(-1, 2, 2)
            if a < 0 or b < 0 or a + b > 1:
                break
    target = p0 + a * e1 + b * e2
    o = (target - 10.0 ** rng.uniform(-1, 3.5) * unit(rng)).astype(np.float32)
    d = target - o.astype(np.float64)
    d = (d / np.linalg.norm(d)).astype(np.float32)
    return np.concatenate([tri[0], tri[1], tri[2], [np.float32(flags)], o, d]).astype(np.float32)


def lattice_rows(rng, per_category=24):
    pow2 = [0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0, -0.25]
    bary = {0: (Fr(0), Fr(0)), 1: (Fr(1), Fr(0)), 2: (Fr(0), Fr(1)), 3: (Fr(0), Fr(1, 2)), 4: (Fr(1, 2), Fr(0)), 5: (Fr(1, 2), Fr(1, 2)), 6: (Fr(1, 4), Fr(1, 4)),
            7: None, 8: (Fr(1, 4), Fr(1, 2))}
    rows, cats = [], []
    for cat in range(len(LATTICE_CATEGORIES)):
        got, tries = 0, 0
        while got < per_category:
            tries += 1
            assert tries < 20000, LATTICE_CATEGORIES[cat]
            p0, e1, e2 = rng.integers(-8, 9, 3), rng.integers(-4, 5, 3), rng.integers(-4, 5, 3)
            if not np.cross(e1, e2).any():
                continue
            flags = int(rng.choice([0, TRI_NOCULL, TRI_FLIP, TRI_NOCULL | TRI_FLIP]))
            if cat <= 8:
                d = rng.choice(pow2, 3)
                if not d.any():
                    continue
                ab = bary[cat] if cat != 7 else [(Fr(-1, 2), Fr(1, 4)), (Fr(3, 4), Fr(3, 4)), (Fr(1, 4), Fr(-1, 4)), (Fr(3, 2), Fr(0))][int(rng.integers(4))]
                s = Fr(int(rng.choice([1, 2, 4]))) * (-1 if cat == 8 else 1)
                o = [Fr(int(p0[k])) + ab[0] * int(e1[k]) + ab[1] * int(e2[k]) - s * fr(d[k]) for k in range(3)]
            else:
                edge = [e1, e2, e2 - e1][int(rng.integers(3))]
                d = (edge if cat == 10 else int(rng.integers(-2, 3)) * e1 + int(rng.integers(-2, 3)) * e2).astype(np.float64) * float(rng.choice([1.0, -1.0, 0.5, 2.0]))
                if not d.any():
                    continue
                start = Fr(int(rng.integers(0, 3)), 2)
                base = p0 + (e1 if (cat == 10 and edge is not e1 and edge is not e2) else 0)
                o = [Fr(int(base[k])) + (start - 2) * fr(d[k]) for k in range(3)]
                if cat == 9 and rng.random() < 0.3:  # parallel to the plane, off it
                    n = np.cross(e1, e2)
                    o = [o[k] + int(n[k]) for k in range(3)]
            if any(rnd(x) != x for x in o):
                continue
            row = np.array([*p0, *e1, *e2, flags, *[float(x) for x in o], *d], np.float32)
            verdict, _, tuv, _, exact_ops = t2_truth(row)
            if not exact_ops:
                continue
            if cat <= 8:
                if tuv is None or (cat != 7 and (tuv[1], tuv[2]) != ab) or (cat == 8) != (tuv[0] < 0):
                    continue
            elif tuv is not None:
                continue
            rows.append(row)
            cats.append(cat)
            got += 1
    return np.array(rows, np.float32), np.array(cats, np.uint8)


def triangle_sets(rng):
    rows, sets = [], []
    four = [0, TRI_NOCULL, TRI_FLIP, TRI_NOCULL | TRI_FLIP]
    for _ in range(1500):
        rows.append(aimed_row(rng, random_triangle(rng), True, TRI_NOCULL if rng.random() < 0.6 else four[int(rng.integers(4))]))
        sets.append(0)
    for _ in range(500):
        rows.append(aimed_row(rng, random_triangle(rng), False, TRI_NOCULL if rng.random() < 0.6 else four[int(rng.integers(4))]))
        sets.append(1)
    for _ in range(600):
        rows.append(aimed_row(rng, random_triangle(rng, sliver=True), True, TRI_NOCULL))
        sets.append(2)
    for flags in four:
        for winding in range(2):
            for _ in range(60):
                p0, e1, e2 = random_triangle(rng)
                rows.append(aimed_row(rng, (p0, e2, e1) if winding else (p0, e1, e2), True, flags))
                sets.append(3)
    lat, cats = lattice_rows(rng)
    rows = np.concatenate([np.array(rows, np.float32), lat])
    sets = np.concatenate([np.array(sets, np.uint8), np.full(len(lat), 4, np.uint8)])
    rows[:, 9] = rows[:, 9].astype(np.uint32).view(np.float32)  # the flags word travels as a bit pattern
    return rows, sets, cats


def triangle_truth(rows, sets):
    n = len(rows)
    verdict, decided, want, bound, detsign = np.zeros(n, bool), np.zeros(n, bool), np.zeros((n, 3)), np.zeros((n, 3), np.float32), np.zeros(n, np.int8)
    for i, r in enumerate(rows):
        x = r.astype(np.float64)
        x[9] = float(r[9:10].view(np.uint32)[0])
        ver, dec, tuv, b, exact_ops = t2_truth(x)
        verdict[i], decided[i] = ver, dec
        if tuv is not None:
            want[i] = [float(q) for q in tuv]
            f = [Fr(float(v)) for v in x]
            pv = [f[14] * f[8] - f[15] * f[7], f[15] * f[6] - f[13] * f[8], f[13] * f[7] - f[14] * f[6]]
            det = f[3] * pv[0] + f[4] * pv[1] + f[5] * pv[2]
            detsign[i] = 1 if det > 0 else -1
        if b is not None:
            bound[i] = [up32(q) for q in b]
        if sets[i] == 4:
            assert exact_ops
            decided[i] = True  # every operation is exact: asserted bit for bit
            bound[i] = 0
    return verdict, decided, want, bound, detsign


def degenerate_triangles(rng):
    sp = np.array([np.inf, -np.inf, np.nan, 1e-45, -1e-40, 3e38, -3e38, 0.0, -0.0, 1e30], np.float32)
    rows = []
    for i in range(240):
        r = aimed_row(rng, random_triangle(rng), True, int(rng.choice([0, 2, 4, 6])))
        kind = i % 4
        if kind == 0:
            r[rng.integers(0, 9, 2)] = rng.choice(sp, 2)
        elif kind == 1:
            r[10 + rng.integers(0, 6, 2)] = rng.choice(sp, 2)
        elif kind == 2:  # repeated vertices: a zero edge, equal edges
            r[3:6] = 0.0 if rng.random() < 0.5 else r[6:9]
        else:
            r[0:9] *= np.float32(1e-38)
        rows.append(r)
    rows = np.array(rows, np.float32)
    rows[:, 9] = rows[:, 9].astype(np.uint32).view(np.float32)
    return rows


# ---- T1 and enter_instance -------------------------------------------------------------------------------------------------------------------------------
def random_affine(rng, translate):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    kind = rng.integers(4)
    if kind == 0:  # axis-aligned, mirrored, with exact zeros of either sign
        q = np.diag(rng.choice([1.0, -1.0], 3))[rng.permutation(3)]
        q = np.where(q == 0, rng.choice([0.0, -0.0], (3, 3)), q)
    m = q * 10.0 ** rng.uniform(-1, 1, 3)[None, :]
    t = 10.0 ** rng.uniform(-1, translate) * unit(rng) if rng.random() < 0.8 else np.zeros(3)
    return np.concatenate([m, t[:, None]], 1).astype(np.float32)  # three rows of four


def world_tri_rows(rng, n=500):
    rows, want = [], []
    for _ in range(n):
        m = random_affine(rng, 3.5)
        v = (10.0 ** rng.uniform(-2, 2) * rng.normal(size=(3, 3)) + (10.0 ** rng.uniform(0, 3) * unit(rng) if rng.random() < 0.3 else 0)).astype(np.float32)
        if rng.random() < 0.1:
            v[rng.integers(3), rng.integers(3)] = rng.choice([0.0, -0.0])
        p = [xform_bits(m, v[k], 1) for k in range(3)]
        e1, e2 = [fsub(p[1][k], p[0][k]) for k in range(3)], [fsub(p[2][k], p[0][k]) for k in range(3)]
        rows.append(np.concatenate([m.reshape(-1), v.reshape(-1)]))
        want.append(p[0] + e1 + e2)
    return np.array(rows, np.float32), np.array(want, np.float32)


def enter_rows(rng, n=400):
    rows, ray, eps = [], [], []
    for _ in range(n):
        m = random_affine(rng, 3.0)
        c0, c1 = np.float32(10.0 ** rng.uniform(-7, -3)), np.float32(10.0 ** rng.uniform(-8, -5))
        o = (10.0 ** rng.uniform(-1, 3) * unit(rng)).astype(np.float32)
        d = unit(rng).astype(np.float32)
        if rng.random() < 0.2:
            d[rng.integers(3)] = rng.choice([0.0, -0.0])
        rows.append(np.concatenate([m.reshape(-1), [c0, c1], o, d]))
        ray.append(xform_bits(m, o, 1) + xform_bits(m, d, 0))
        eps.append(float(fr(c1) * max(abs(fr(x)) for x in o) + fr(c0)))
    return np.array(rows, np.float32), np.array(ray, np.float32), np.array(eps, np.float64)


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------------------------
def exact_interval(lo, hi, o, d, lim):
    """[tmin, tmax] of the t in [0, lim] with o + t d inside [lo, hi], or None"""
    tmin, tmax = Fr(0), lim
    for a in range(3):
        if d[a] == 0:
            if not lo[a] <= o[a] <= hi[a]:
                return None
            continue
        t1, t2 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        if t1 > t2:
            t1, t2 = t2, t1
        tmin, tmax = max(tmin, t1), min(tmax, t2)
    return (tmin, tmax) if tmin <= tmax else None


def entry_param(lo, hi, o, d):
    """max(0, the largest near-plane parameter): the entry distance where the ray meets the box"""
    t = Fr(0)
    for a in range(3):
        if d[a] != 0:
            t = max(t, min((lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]))
    return t


def node_rows(rng, n=2200):
    specials = np.array([0.0, -0.0, 1e-30, -1e-20, 1e-10], np.float32)
    rows = np.zeros((n, 36), np.float32)
    for i in range(n):
        base = 10.0 ** rng.uniform(0, 4) * unit(rng) if rng.random() < 0.5 else np.zeros(3)
        spread = 10.0 ** rng.uniform(-1, 1.5)
        cluster = 0.25 if rng.random() < 0.6 else 1.0  # clustered children overlap, so that a visit has several hits to put in order
        lo, hi, words = np.full((4, 3), FLT_MAX, np.float32), np.full((4, 3), -FLT_MAX, np.float32), np.full(4, BVH_NONE, np.uint32)
        empty = rng.random(4) < 0.25
        if empty.all():
            empty[rng.integers(4)] = False
        grid = rng.random() < 0.15  # integer planes on a node whose grid step is 1: the compact form holds every plane exactly, nothing but its bias protects a graze
        if grid:
            gp, ge = rng.integers(-1500, -200, 3), rng.integers(1025, 2048, 3)
            base, spread = (gp + ge / 2).astype(np.float64), 300.0
        real = np.flatnonzero(~empty)
        for k in real:
            if grid:
                l = gp + rng.integers(0, ge)
                h = l + (rng.integers(0, gp + ge - l + 1) if rng.random() < 0.8 else 0)
                if k == real[0]:
                    l = gp.copy()
                if k == real[-1]:
                    h = gp + ge
                lo[k], hi[k] = l.astype(np.float32), np.maximum(l, h).astype(np.float32)
            else:
                c, h = base + cluster * spread * rng.normal(size=3), spread * 10.0 ** rng.uniform(-1.5, 0.4, 3)
                flat = rng.random()
                if flat < 0.3:
                    h[rng.integers(3)] = 0.0
                elif flat < 0.45:
                    h[rng.permutation(3)[:2]] = 0.0
                lo[k], hi[k] = (c - h).astype(np.float32), (c + h).astype(np.float32)
                hi[k] = np.maximum(lo[k], hi[k])
            words[k] = (BVH_LEAF if rng.random() < 0.5 else 0) | (BVH_ALPHA if rng.random() < 0.5 else 0) | (1000 + 4 * i + k)
        k = int(rng.choice(np.flatnonzero(~empty)))  # the child the ray is aimed at
        blo, bhi = lo[k].astype(np.float64), hi[k].astype(np.float64)
        where = rng.integers(2) if grid else rng.integers(4)  # origin inside the box, near, far, at (or next to) the world's origin with the boxes far from it
        what = rng.integers(4) if where != 3 else rng.integers(2)  # corner, face, interior, beside the box
        w = rng.random(3)
        target = blo + w * (bhi - blo)
        if what == 0:
            target = np.where(rng.random(3) < 0.5, blo, bhi)
        elif what == 1:
            a = rng.integers(3)
            target[a] = blo[a] if rng.random() < 0.5 else bhi[a]
        elif what == 3:
            a = rng.integers(3)
            target[a] = bhi[a] + (bhi[a] - blo[a] + 1e-3 * spread) * rng.uniform(0.001, 2.0)
        dist = 0.0 if where == 0 else 10.0 ** (rng.uniform(-2, 1) if where == 1 else rng.uniform(1, 4))
        dirn = unit(rng)
        o = (target - dist * dirn).astype(np.float32) if where else (blo + rng.random(3) * (bhi - blo)).astype(np.float32)
        if where == 3:  # o idir is (nearly) zero: the bias of n vanishes and the (1 -+ 4e-7) factors alone keep the test conservative
            o = (np.zeros(3) if rng.random() < 0.5 else 1e-3 * spread * rng.normal(size=3)).astype(np.float32)
        d = target - o.astype(np.float64)
        d = (d / np.linalg.norm(d)).astype(np.float32) if np.linalg.norm(d) > 0 else dirn.astype(np.float32)
        mode = rng.random()
        if mode < 0.45:  # one or two components take a special value; the origin then sits in (or exactly on the planes of) the target's slab
            for a in rng.permutation(3)[:int(rng.integers(1, 3))]:
                d[a] = rng.choice(specials)
                pick = rng.integers(4)
                o[a] = [lo[k][a], hi[k][a], np.float32(0.5 * (blo[a] + bhi[a])), o[a]][pick]
            if np.abs(d).max() < 0.5:
                d[np.argmax(np.abs(d))] = np.float32(rng.choice([1.0, -1.0]))
        lim_kind = rng.random()
        lim = np.float32(3e38)
        if lim_kind < 0.15:
            lim = np.float32(0.0)
        elif lim_kind < (0.40 if where != 3 else 0.65):
            q = entry_param([fr(x) for x in lo[k]], [fr(x) for x in hi[k]], [fr(x) for x in o], [fr(x) for x in d])
            lim = np.float32(float(q))  # the exact entry distance, rounded to nearest or (half of the rows) up: then the exact interval is one point wide
            if rng.random() < 0.5 and fr(lim) < q:
                lim = np.nextafter(lim, np.float32(np.inf))
        rows[i, 0:12] = lo.T.reshape(-1)
        rows[i, 12:24] = hi.T.reshape(-1)
        rows[i, 24:28] = words.view(np.float32)
        rows[i, 28:31], rows[i, 31:34], rows[i, 34] = o, d, lim
        rows[i, 35:36] = np.array([1 if rng.random() < 0.25 else 0], np.uint32).view(np.float32)
    return rows


def node_truth(rows):
    """per row and child: must (exact interval non-empty, real child, alpha filter), may / may_c (the same against the grown box, wide / compact form), and the
    entry distance's range: entry_hi (exact box), entry_lo / entry_lo_c (grown boxes, times 1 - REL)"""
    n = len(rows)
    must, may, may_c = np.zeros((n, 4), bool), np.zeros((n, 4), bool), np.zeros((n, 4), bool)
    e_hi, e_lo, e_lo_c = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    for i, r in enumerate(rows):
        words = r[24:28].view(np.uint32)
        alpha_only = r[35:36].view(np.uint32)[0] != 0
        o, d, lim = [fr(x) for x in r[28:31]], [fr(x) for x in r[31:34]], fr(r[34])
        lo = [[fr(r[4 * a + k]) for a in range(3)] for k in range(4)]
        hi = [[fr(r[12 + 4 * a + k]) for a in range(3)] for k in range(4)]
        real = [k for k in range(4) if words[k] != BVH_NONE]
        m = max(range(3), key=lambda a: abs(d[a]))
        m_all = [max(max(abs(lo[k][a]), abs(hi[k][a])) for k in real) for a in range(3)]
        step, org = [], []
        for a in range(3):
            p = min(lo[k][a] for k in real)
            ext = max(hi[k][a] for k in real) - p
            e = 27
            while GRID * Fr(2) ** (e - 127) < ext:
                e += 1
            step.append(Fr(2) ** (e - 127))
            org.append(p)
        for k in real:
            if alpha_only and not (words[k] & BVH_ALPHA):
                continue
            clamp = [CLAMP_D * (abs(o[m]) + max(abs(lo[k][m]), abs(hi[k][m]))) * (1 + Fr(1, 10 ** 5)) / abs(d[m]) if abs(d[a]) < CLAMP_D else Fr(0) for a in range(3)]
            mk = [max(abs(lo[k][a]), abs(hi[k][a])) for a in range(3)]
            g = [BETA * abs(o[a]) + REL * (abs(o[a]) + mk[a]) + clamp[a] for a in range(3)]
            gc = [step[a] + BETA * abs(o[a]) + CB * (abs(org[a] - o[a]) + BETA * abs(o[a]) + GRID * step[a]) + REL * (abs(o[a]) + mk[a] + step[a]) + clamp[a] for a in range(3)]
            must[i, k] = exact_interval(lo[k], hi[k], o, d, lim) is not None
            glo, ghi = [lo[k][a] - g[a] for a in range(3)], [hi[k][a] + g[a] for a in range(3)]
            clo, chi = [lo[k][a] - gc[a] for a in range(3)], [hi[k][a] + gc[a] for a in range(3)]
            may[i, k] = exact_interval(glo, ghi, o, d, lim * (1 + REL)) is not None
            may_c[i, k] = exact_interval(clo, chi, o, d, lim * (1 + REL)) is not None
            assert may[i, k] >= must[i, k] and may_c[i, k] >= may[i, k]
            hi_q = entry_param(lo[k], hi[k], o, d)
            e_hi[i, k] = up32(min(hi_q, Fr(3 * 10 ** 38)))
            e_lo[i, k] = -up32(-min(entry_param(glo, ghi, o, d), Fr(3 * 10 ** 38)) * (1 - REL) * (1 - Fr(1, 1 << 19)))
            e_lo_c[i, k] = -up32(-min(entry_param(clo, chi, o, d), Fr(3 * 10 ** 38)) * (1 - REL) * (1 - Fr(1, 1 << 19)))
    return must, may, may_c, e_hi, e_lo, e_lo_c


def degenerate_nodes(rng, rows):
    sp = np.array([np.inf, -np.inf, np.nan, 1e-45, -1e-40, 3e38, -3e38, 1e30, -1e25, 0.0], np.float32)
    out = rows[rng.permutation(len(rows))[:240]].copy()
    for i, r in enumerate(out):
        kind = i % 3
        if kind == 0:
            r[rng.integers(0, 24, 3)] = rng.choice(sp, 3)
        elif kind == 1:
            r[28 + rng.integers(0, 6, 2)] = rng.choice(sp, 2)
        else:
            with np.errstate(over="ignore"):
                r[0:24] *= np.float32(1e25)
                r[28:31] *= np.float32(1e25)
        if i % 5 == 0:
            r[34] = rng.choice(np.array([np.nan, np.inf, -1.0], np.float32))
    return out


def build():
    rng = np.random.default_rng(20251018)
    tri_in, tri_set, lattice_cat = triangle_sets(rng)
    verdict, decided, want, bound, detsign = triangle_truth(tri_in, tri_set)
    wt_in, wt_want = world_tri_rows(rng)
    en_in, en_ray, en_eps = enter_rows(rng)
    nd_in = node_rows(rng)
    must, may, may_c, e_hi, e_lo, e_lo_c = node_truth(nd_in)
    return dict(tri_in=tri_in, tri_set=tri_set, lattice_cat=lattice_cat, tri_verdict=verdict, tri_decided=decided, tri_want=want, tri_bound=bound, tri_detsign=detsign,
                tri_degenerate=degenerate_triangles(rng), world_tri_in=wt_in, world_tri_want=wt_want, enter_in=en_in, enter_ray=en_ray, enter_eps=en_eps, node_in=nd_in,
                node_must=must, node_may=may, node_may_c=may_c, node_entry_hi=e_hi, node_entry_lo=e_lo, node_entry_lo_c=e_lo_c, node_degenerate=degenerate_nodes(rng, nd_in))


def write(path, arrays):
    """np.savez_compressed with fixed member times: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    kat = build()
    write(sys.argv[1] if len(sys.argv) > 1 else OUT, kat)
    for s, name in enumerate(SETS):
        m = kat["tri_set"] == s
        print(f"{name:9s} {m.sum():5d} rows, undecided {1 - kat['tri_decided'][m].mean():.3f}, exact hits {kat['tri_verdict'][m].mean():.3f}")
    print("node rows", len(kat["node_in"]), "exact hits", int(kat["node_must"].sum()), "may", int(kat["node_may"].sum()), "may (compact)", int(kat["node_may_c"].sum()))
